"""One fixed sequence of session calls that touches every buffer a session
keeps between calls (tests/test_gpu_lifecycle.py compares it across viewport
sizes; tools/alloc_calls.py counts its allocation calls): the frame and the
lanes (compute), first_hit's planes and spill, denoise's scratch, both kept
histories and the merged frame (two keeping reprojects around a camera move),
sample_map's scratch and compute_map's plan, the scaled first-hit planes and
upsample's outputs (scale 2 from the merged frame after the filter has reused
its scratch, then scale 3: both grow within one viewport)."""
import numpy as np

SEED = 0xBABABEBE
DEPTH = 4
KEEP = 1  # WPT_REPROJECT_KEEP
MERGED = 1  # WPT_UPSAMPLE_MERGED
# the first viewport; one that grows every grow-only buffer, with an odd pixel
# count (777 pixels: no plane is a multiple of 256 B); one below both
SIZES = ((24, 16), (37, 21), (8, 8))


def mesh(pkg):
    return pkg.scenes.triangle_cloud(3000, seed=0x5EED)


def cameras(pkg):
    a = tuple(pkg.scenes.scene_camera(2))
    return a, (a[0] + 0.25,) + a[1:]


def start(itf, pkg, tris, vp):
    """A fresh session of scene 2 with `tris` at viewport vp: NEE on both
    halves, random sampling."""
    itf.init(vp[0], vp[1], 2, *cameras(pkg)[0])
    assert itf.store_mesh(1, tris)
    itf.update_settings(1, 1, 0, 0, 0)
    itf.set_render_options(DEPTH, SEED, 0)


def calls(itf, pkg, vp):
    """The sequence at the session's viewport vp, from camera A on: a list of
    (name, array) of everything the calls return."""
    cam_a, cam_b = cameras(pkg)
    npx = vp[0] * vp[1]
    out = []

    def keep(name, arrays):
        out.extend((f"{name}[{i}]", np.ascontiguousarray(a)) for i, a in enumerate(arrays))

    itf.update_camera(*cam_a)  # (resets the accumulation: every run of the sequence starts alike)
    itf.compute(3 * npx)
    fh = itf.first_hit(0)
    keep("first_hit", [fh[k] for k in sorted(fh)])
    keep("denoise", itf.denoise(0))
    keep("reproject_keep_a", itf.reproject(0, flags=KEEP))
    itf.update_camera(*cam_b)
    itf.compute(npx)
    keep("reproject_keep_b", itf.reproject(0, flags=KEEP))
    keep("denoise_merged", itf.denoise_merged())
    keep("upsample_merged", itf.upsample(2, 0, iterations=3, flags=MERGED))
    count, totals = itf.sample_map(0, target=6, max_per_pixel=4)
    keep("sample_map", [count, np.array(totals, dtype=np.uint64)])
    itf.compute_map(None)
    keep("upsample", itf.upsample(3, 0, iterations=0))
    keep("read_radiance", itf.read_radiance(*vp))
    return out
