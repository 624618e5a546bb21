"""Python mirror of the reference's operator interface, src/wasm_interface.rs.

Same function names and argument meaning as the reference's wasm exports
(init, results, update_scene, update_settings, update_viewport,
update_camera, allocate_mesh, mesh_vertices, notify_mesh_loaded,
allocate_texture, notify_texture_loaded, compute). Where the reference
panics (a WASM trap) these raise ``WptError`` carrying the library's status
code and message. Everything runs through libwpt.so; nothing here computes.
"""
import ctypes

import numpy as np

from ._lib import lib

OK = 0
ERR_NOT_INIT, ERR_ALREADY_INIT, ERR_INVALID_SCENE, ERR_INVALID_ARG = -1, -2, -3, -4
ERR_UNSUPPORTED, ERR_DEVICE, ERR_NO_MESH = -5, -6, -7
NO_NEE, NORMAL_NEE, PNEE = 0, 1, 2


class WptError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def _check(rc):
    if rc < 0:
        raise WptError(rc, lib().wpt_last_error().decode())
    return rc


# ---- reference exports (wasm_interface.rs) ---------------------------------
def init(width, height, scene_id, cam_x, cam_y, cam_z, cam_rot_x, cam_rot_y):
    """wasm_interface.rs:67"""
    _check(lib().wpt_init(width, height, scene_id, cam_x, cam_y, cam_z, cam_rot_x, cam_rot_y))


def results(is_show_sampling=0, width=None, height=None):
    """wasm_interface.rs:120 — returns a (H, W, 4) uint8 copy of the buffer."""
    p = lib().wpt_results(is_show_sampling)
    if not p:
        raise WptError(ERR_NOT_INIT, lib().wpt_last_error().decode())
    n = width * height * 4
    return np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(height, width, 4)


def update_scene(scene_id):
    """wasm_interface.rs:154"""
    _check(lib().wpt_update_scene(scene_id))


def update_settings(left_type, right_type, is_left_adaptive, is_right_adaptive, is_light_debug):
    """wasm_interface.rs:173"""
    _check(lib().wpt_update_settings(left_type, right_type, is_left_adaptive, is_right_adaptive, is_light_debug))


def update_viewport(width, height):
    """wasm_interface.rs:219"""
    _check(lib().wpt_update_viewport(width, height))


def update_camera(cam_x, cam_y, cam_z, cam_rot_x, cam_rot_y):
    """wasm_interface.rs:239"""
    _check(lib().wpt_update_camera(cam_x, cam_y, cam_z, cam_rot_x, cam_rot_y))


def allocate_mesh(mesh_id, num_vertices):
    """wasm_interface.rs:259"""
    _check(lib().wpt_allocate_mesh(mesh_id, num_vertices))


def mesh_vertices(mesh_id, num_vertices):
    """wasm_interface.rs:275 — a writable (num_vertices, 3) float32 view."""
    p = lib().wpt_mesh_vertices(mesh_id)
    if not p:
        raise WptError(ERR_NO_MESH, lib().wpt_last_error().decode())
    return np.ctypeslib.as_array(p, shape=(num_vertices * 3,)).reshape(num_vertices, 3)


def notify_mesh_loaded(mesh_id):
    """wasm_interface.rs:293 — True if the active scene was rebuilt."""
    return bool(_check(lib().wpt_notify_mesh_loaded(mesh_id)))


def _obj_args(text, scale):
    b = text.encode() if isinstance(text, str) else bytes(text)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    return b, sc, (None if sc is None else sc.ctypes.data)


def parse_obj(text, scale=None):
    """obj_parser.ts:3-51 in libwpt.so (wpt_parse_obj, host only): float32
    (3 * vertices,) triangle soup, scaled per axis if `scale` is given."""
    b, sc, sp = _obj_args(text, scale)
    n = ctypes.c_uint64(0)
    _check(lib().wpt_parse_obj(b, len(b), sp, None, 0, ctypes.addressof(n)))
    out = np.empty(3 * n.value, dtype=np.float32)
    _check(lib().wpt_parse_obj(b, len(b), sp, out.ctypes.data if n.value else None, n.value, ctypes.addressof(n)))
    return out


def load_obj(mesh_id, text, scale=None):
    """OBJ text into mesh slot `mesh_id` (wpt_load_obj); then call
    notify_mesh_loaded(mesh_id). Returns the vertex count."""
    b, sc, sp = _obj_args(text, scale)
    n = ctypes.c_uint64(0)
    _check(lib().wpt_load_obj(mesh_id, b, len(b), sp, ctypes.addressof(n)))
    return n.value


def allocate_texture(tex_id, width, height):
    """wasm_interface.rs:335"""
    p = lib().wpt_allocate_texture(tex_id, width, height)
    if not p:
        raise WptError(ERR_NOT_INIT, lib().wpt_last_error().decode())
    return np.ctypeslib.as_array(p, shape=(width * height * 3,))


def notify_texture_loaded(tex_id):
    """wasm_interface.rs:358 (always False)"""
    return bool(_check(lib().wpt_notify_texture_loaded(tex_id)))


def compute(num_samples):
    """wasm_interface.rs:374"""
    _check(lib().wpt_compute(num_samples))


# ---- additions --------------------------------------------------------------
def store_mesh(mesh_id, vertices):
    """The worker's mesh upload protocol (worker.ts:171-179):
    allocate_mesh → fill mesh_vertices → notify_mesh_loaded."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    allocate_mesh(mesh_id, v.shape[0])
    mesh_vertices(mesh_id, v.shape[0])[:] = v
    return notify_mesh_loaded(mesh_id)


def set_device(dev):
    _check(lib().wpt_set_device(dev))


def set_render_options(max_depth=0, frame_seed=0xBABABEBE, batch_paths=0):
    _check(lib().wpt_set_render_options(max_depth, frame_seed, batch_paths))


def set_partition(rank, nranks, tile=16):
    _check(lib().wpt_set_partition(rank, nranks, tile))


def partition_pixels():
    n = _check(lib().wpt_partition_pixels(None))
    out = np.empty(n, dtype=np.uint32)
    _check(lib().wpt_partition_pixels(out.ctypes.data))
    return out


def tile_partition(width, height, rank, nranks, tile=16):
    """Host-only: pixel indices set_partition(rank, nranks, tile) would give."""
    n = _check(lib().wpt_tile_partition(width, height, rank, nranks, tile, None))
    out = np.empty(n, dtype=np.uint32)
    _check(lib().wpt_tile_partition(width, height, rank, nranks, tile, out.ctypes.data))
    return out


def photon_tree(num_lights):
    """Frozen PNEE octree: (child[nodes], cum[nodes, num_lights], shot, stored)."""
    n = _check(lib().wpt_photon_tree(None, None, None))
    child = np.empty(n, dtype=np.uint32)
    cum = np.empty(n * max(num_lights, 1), dtype=np.float32)
    ss = np.empty(2, dtype=np.uint64)
    _check(lib().wpt_photon_tree(child.ctypes.data, cum.ctypes.data, ss.ctypes.data))
    return child, cum[: n * num_lights].reshape(n, num_lights), int(ss[0]), int(ss[1])


def _photon_arrays(photons):
    light, loc, intensity = photons
    li = np.ascontiguousarray(light, dtype=np.uint32)
    lo = np.ascontiguousarray(loc, dtype=np.float32).reshape(-1, 3)
    it = np.ascontiguousarray(intensity, dtype=np.float32)
    assert li.shape[0] == lo.shape[0] == it.shape[0]
    return li, lo, it


def photon_build(num_lights, photons):
    """Host-only: the frozen octree of a photon list (light ids, locations
    (n, 3), intensities; insertion order): (child[nodes], cum[nodes,
    num_lights], corners[nodes, 8, 8]) (wpt_photon_build)."""
    li, lo, it = _photon_arrays(photons)
    L = lib()
    args = (num_lights, li.shape[0], li.ctypes.data, lo.ctypes.data, it.ctypes.data)
    n = _check(L.wpt_photon_build(*args, None, None, None))
    child = np.empty(n, dtype=np.uint32)
    cum = np.empty(n * max(num_lights, 1), dtype=np.float32)
    corners = np.empty((n, 8, 8), dtype=np.uint32)
    _check(L.wpt_photon_build(*args, child.ctypes.data, cum.ctypes.data, corners.ctypes.data))
    return child, cum[: n * num_lights].reshape(n, num_lights), corners


def install_photons(photons):
    """Test hook: the photon list as the session's PNEE octree, until a new
    scene or frame seed drops it (wpt_install_photons)."""
    li, lo, it = _photon_arrays(photons)
    _check(lib().wpt_install_photons(li.shape[0], li.ctypes.data, lo.ctypes.data, it.ctypes.data))


def photon_sample(points, states, view, table=True):
    """Test hook: the device's PhotonTree::sample of points (n, 3), point i on
    the xorshift32 state states[i], reading the octree as the shade kernel's
    variant `view` (0, 1, 2) does: (light, pdf, state after) per point."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    s = np.ascontiguousarray(states, dtype=np.uint32)
    n = p.shape[0]
    assert s.shape == (n,)
    light = np.empty(n, dtype=np.uint32)
    pdf = np.empty(n, dtype=np.float32)
    out = np.empty(n, dtype=np.uint32)
    _check(lib().wpt_photon_sample(n, p.ctypes.data, s.ctypes.data, int(view), 1 if table else 0, light.ctypes.data,
                                   pdf.ctypes.data, out.ctypes.data))
    return light, pdf, out


def adaptive_error(acc, cnt, half):
    """Test hook: the error estimate of an adaptive round on the frame acc
    (H, W, 3) f32 sums / cnt (H, W) u32 counts, through the session's planner
    kernels and host walk: (errors of screen half `half` (H, its width), f32
    {sum, min, max})."""
    a = np.ascontiguousarray(acc, dtype=np.float32)
    c = np.ascontiguousarray(cnt, dtype=np.uint32)
    H, W = c.shape
    assert a.shape == (H, W, 3)
    rw = W - W // 2 if half else W // 2
    mse = np.empty((H, rw), dtype=np.float32)
    stats = np.empty(3, dtype=np.float32)
    _check(lib().wpt_adaptive_error(W, H, a.ctypes.data, c.ctypes.data, int(half), mse.ctypes.data, stats.ctypes.data))
    return mse, stats


def adaptive_plan(width, height, half, mse, stats, cnt, samp, first=False, adaptive=True):
    """Test hook: the planning part of a round of screen half `half` from the
    caller's errors, {sum, min, max} and counts: (count (H, W), offset
    (W*H + 1), base (H, W), the sampling view (H, W, 4) u8; samp is not
    modified)."""
    m = np.ascontiguousarray(mse, dtype=np.float32)
    s = np.ascontiguousarray(stats, dtype=np.float32)
    c = np.ascontiguousarray(cnt, dtype=np.uint32)
    view = np.array(samp, dtype=np.uint8, order="C", copy=True)
    rw = width - width // 2 if half else width // 2
    assert m.size == height * rw and s.shape == (3,)
    assert c.size == width * height and view.size == 4 * width * height
    count = np.empty((height, width), dtype=np.uint32)
    offset = np.empty(width * height + 1, dtype=np.uint32)
    base = np.empty((height, width), dtype=np.uint32)
    _check(lib().wpt_adaptive_plan(width, height, int(half), int(bool(first)), int(bool(adaptive)), m.ctypes.data,
                                   s.ctypes.data, c.ctypes.data, count.ctypes.data, offset.ctypes.data,
                                   base.ctypes.data, view.ctypes.data))
    return count, offset, base, view.reshape(height, width, 4)


def read_radiance(width, height):
    acc = np.empty(width * height * 3, dtype=np.float32)
    cnt = np.empty(width * height, dtype=np.uint32)
    _check(lib().wpt_read_radiance(acc.ctypes.data, cnt.ctypes.data))
    return acc.reshape(height, width, 3), cnt.reshape(height, width)


def comm_unique_id():
    """ncclGetUniqueId (128 bytes): made on one rank, handed to every rank."""
    buf = ctypes.create_string_buffer(128)
    _check(lib().wpt_comm_unique_id(buf))
    return buf.raw


def set_comm(rank, nranks, tile, unique_id):
    """Collective: this rank's tile partition plus an RCCL communicator over
    all ranks; adaptive rounds then exchange the frame over it."""
    uid = ctypes.create_string_buffer(bytes(unique_id), 128)
    _check(lib().wpt_set_comm(rank, nranks, tile, uid))


def gather_frame(root=0):
    """Collective: every rank's partition into root's frame (RCCL over xGMI)."""
    _check(lib().wpt_gather_frame(root))


def gather_plan(rank, nranks, root, slot):
    """Host-only: the rooted gather's point-to-point transfers as `rank`
    posts them: (peer, float4 offset in root's buffer, float4 count, recv)."""
    n = _check(lib().wpt_gather_plan(rank, nranks, root, slot, None))
    out = np.zeros(4 * max(n, 1), dtype=np.uint64)
    _check(lib().wpt_gather_plan(rank, nranks, root, slot, out.ctypes.data))
    return [(int(a), int(b), int(c), bool(d)) for a, b, c, d in out[: 4 * n].reshape(-1, 4)]


def comm_destroy():
    _check(lib().wpt_comm_destroy())


def copy_partition(device_ptr):
    _check(lib().wpt_copy_partition(ctypes.c_void_p(device_ptr)))


def stats():
    keys = ("paths", "rays", "shadow_rays", "node_visits", "prim_tests", "bounces", "ext_visits", "ext_tests",
            "ext_node_bytes", "sh_visits", "sh_tests", "sh_node_bytes", "fallback_ext", "fallback_sh",
            "ext_lane_iters", "ext_live_iters", "sh_lane_iters", "sh_live_iters", "photon_rays", "photons",
            "sum_chunks", "sum_resummed", "sum_fetched", "stock_consumed", "fill_paths", "trace_bytes",
            "finish_paths", "finish_max_bounces", "max_ray_visits", "ex_body_lanes", "ex_bodies", "lf_body_lanes",
            "lf_bodies", "stock_traced", "stock_deficit", "stock_waits", "plan_us", "stock_us",
            "stock_rays", "stock_rays_used", "presolved_rays", "dropped_rays",
            "shadow_presolved_rays", "gen_shaded_rays")
    out = (ctypes.c_uint64 * len(keys))()
    _check(lib().wpt_stats(ctypes.addressof(out), len(keys)))
    return dict(zip(keys, list(out)))


def kernel_times():
    """Per kernel: summed launch ms and launches, and (the lanes' launches
    overlap) busy_ms = union of the launch intervals, logical launches = one
    per bounce (generate / accumulate: one per batch)."""
    out = (ctypes.c_double * 28)()
    _check(lib().wpt_kernel_times(ctypes.addressof(out), 28))
    names = ("generate", "extend", "shade", "shadow", "accumulate", "trace")  # trace: fused extend + shadow
    kt = {n: {"ms": out[2 * i], "launches": int(out[2 * i + 1]), "busy_ms": out[12 + 2 * i],
              "logical_launches": int(out[13 + 2 * i])} for i, n in enumerate(names)}
    return kt


def set_counting(on):
    _check(lib().wpt_set_counting(1 if on else 0))


def set_profiling(on):
    _check(lib().wpt_set_profiling(1 if on else 0))


def scene_build_info():
    """The active scene's BVH2 build: (ms, built on the GPU)."""
    out = (ctypes.c_double * 2)()
    _check(lib().wpt_scene_build_info(ctypes.addressof(out)))
    return float(out[0]), bool(out[1])


def set_lanes(n):
    """Concurrent lanes of the next compute calls (1 serialises the kernels)."""
    _check(lib().wpt_set_lanes(int(n)))


# launch configuration (include/wpt.h WPT_OPT_*): no environment variable
# changes it; the frame is bit-identical for every setting
OPTIONS = {"defaults": 0, "traversal": 1, "traversal_sh": 2, "fused": 3, "fused_below": 4, "small_lanes": 5, "pixel_tile": 6,
           "grid_pct": 7, "refill": 8, "refill_sh": 9, "treelet": 10, "bvh_build": 11, "lanes": 12,
           "finish_below": 13, "trace_grid_pct": 14, "finish_every": 20, "probe": 22, "stock": 23, "stock_lanes": 24,
           "fill": 25, "async_prio": 26, "async_grid_pct": 27, "scene_traversal": 28, "scene_tri_only": 29,
           "stock_ahead": 30, "async_oneshot": 31, "stock_every": 32, "stock_extra": 33,
           "log": 34, "stock_prefill": 35, "async_fused_below": 36, "presolve": 37, "drop_miss": 38,
           "presolve_shadow": 39, "gen_shade": 40, "oct_view": 41,
           "stock_ranks": 42, "stock_ring_bytes": 43, "viewport": 44,
           "denoise_lds": 45, "history": 46, "map_mode": 47}
# symbolic values of the enumerated options
# traversal: exact BVH2, the BVH4 fast path, or auto (the default: BVH4 on
# scenes with other shapes than triangles, else BVH2)
TRAVERSALS = {"bvh2": 0, "bvh4": 1, "auto": 3}
OPTION_VALUES = {"traversal": TRAVERSALS, "traversal_sh": TRAVERSALS,
                 "bvh_build": {"auto": 0, "host": 1, "gpu": 2}}


def set_option(name, value):
    """wpt_set_option: with no session the default of every later init
    (set_option("defaults", 0) restores the built-in ones), with a session
    that session only (scene / partition rebuilt where the option shapes it)."""
    if isinstance(value, str) and not value.lstrip("-").isdigit():
        value = OPTION_VALUES[name][value]
    _check(lib().wpt_set_option(OPTIONS[name], int(value)))


def get_option(name):
    v = ctypes.c_int64(0)
    _check(lib().wpt_get_option(OPTIONS[name], ctypes.addressof(v)))
    return v.value


def probe_read():
    """Wave timelines recorded since set_option("probe", N) (wpt_probe_read):
    (meta, rec, ticks_per_us): meta (launches, 5) u32 = kernel (1 extend,
    3 shadow, 5 trace), lane, bounce, waves, first entry; rec (entries, 4) u32
    = start, feed dry, end (steady-clock ticks), rays taken."""
    L = lib()
    ent = ctypes.c_uint64(0)
    tpu = ctypes.c_double(0.0)
    n = L.wpt_probe_read(None, None, ctypes.addressof(ent), ctypes.addressof(tpu))
    if n < 0:
        raise WptError(int(n), L.wpt_last_error().decode())
    meta = np.zeros((n, 5), np.uint32)
    rec = np.zeros((ent.value, 4), np.uint32)
    if n:
        ent.value = rec.shape[0]  # rec's capacity (entries)
        _check(L.wpt_probe_read(meta.ctypes.data, rec.ctypes.data, ctypes.addressof(ent), ctypes.addressof(tpu)))
    return meta, rec, tpu.value


def clear_stats():
    _check(lib().wpt_clear_stats())


def sync():
    _check(lib().wpt_sync())


def bvh_depth():
    return _check(lib().wpt_bvh_depth())


def trace_rays(rays):
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = r.shape[0]
    t = np.empty(n, dtype=np.float32)
    ids = np.empty(n, dtype=np.int32)
    _check(lib().wpt_trace_rays(n, r.ctypes.data, t.ctypes.data, ids.ctypes.data))
    return t, ids


def shadow_rays(pq, light_ids):
    p = np.ascontiguousarray(pq, dtype=np.float32).reshape(-1, 6)
    li = np.ascontiguousarray(light_ids, dtype=np.int32)
    occ = np.empty(p.shape[0], dtype=np.uint8)
    _check(lib().wpt_shadow_rays(p.shape[0], p.ctypes.data, li.ctypes.data, occ.ctypes.data))
    return occ.astype(bool)


FIRST_HIT_PLANES = {  # name -> (argument position in wpt_first_hit, dtype, components)
    "dir": (0, np.float32, 3), "t": (1, np.float32, 1), "id": (2, np.int32, 1), "visits": (3, np.uint32, 1),
    "normal": (4, np.float32, 3), "albedo": (5, np.float32, 3), "kind": (6, np.uint8, 1),
}


def first_hit(sample=0, planes=("dir", "t", "id", "visits", "normal", "albedo", "kind")):
    """First-hit feature planes of sample `sample` of every frame pixel
    (wpt_first_hit): a dict plane name -> (H, W) or (H, W, 3) array of the
    planes asked for. t is +inf and id -1 on a miss; kind is 0 miss, 1 diffuse,
    2 emissive."""
    vp = get_option("viewport")
    w, h = vp & 0xFFFFFFFF, vp >> 32
    out, ptr = {}, [None] * 7
    for name in planes:
        pos, dt, c = FIRST_HIT_PLANES[name]
        out[name] = np.empty((h, w, 3) if c == 3 else (h, w), dtype=dt)
        ptr[pos] = out[name].ctypes.data
    _check(lib().wpt_first_hit(sample, *ptr))
    return out


def primary_rays(width, height, cam, seed=0xBABABEBE, sample=0):
    """The primary rays of a width x height frame as the generate kernels make
    them (wpt_primary_rays; host only, no session): (height * width, 6) f32
    {origin, direction} in raster order. cam = (x, y, z, rot_x, rot_y)."""
    c = np.ascontiguousarray(cam, dtype=np.float32).reshape(5)
    rays = np.empty((width * height, 6), dtype=np.float32)
    _check(lib().wpt_primary_rays(width, height, c.ctypes.data, seed, sample, rays.ctypes.data))
    return rays


RAYS_DEVICE = 1  # WPT_RAYS_DEVICE: radiance_rays' arrays are device pointers


def radiance_rays(rays, keys=None, sample=0, spp=1, type=1, device=False):
    """Path-traced radiance along a caller's rays (wpt_radiance_rays): ray i =
    rays[i] = {origin, direction}, its samples sample .. sample + spp - 1 on
    the streams of keys[i] (None: i), as camera paths of render type `type`
    under the session's scene and render options. Returns (rgb (n, 3) f32: the
    sum over the ray's samples in sample order, status (n,) u8: 0 for a ray
    with a non-finite component or a zero direction, which is not traced).
    device=True: rays (n, 6) f32 and keys (n,) i32 / u32 bits are contiguous
    torch tensors on the session's device, and so are the results (status as
    torch.uint8); the call still returns synchronised. The session's frame,
    rounds, stock and map are not touched."""
    if device:
        import torch

        if rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 6:
            raise ValueError("rays: a contiguous float32 tensor of 6 components per ray")
        n = rays.numel() // 6
        if keys is not None and (keys.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                                 or not keys.is_contiguous()
                                 or keys.numel() != n or keys.device != rays.device):
            raise ValueError("keys: a contiguous 32-bit integer tensor of one key per ray, on the rays' device")
        rgb = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
        status = torch.empty((n,), dtype=torch.uint8, device=rays.device)
        _check(lib().wpt_radiance_rays(n, rays.data_ptr(), keys.data_ptr() if keys is not None else None, sample, spp,
                                       type, RAYS_DEVICE, rgb.data_ptr(), status.data_ptr()))
        return rgb, status
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = r.shape[0]
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint32).reshape(n)
    rgb = np.empty((n, 3), dtype=np.float32)
    status = np.empty(n, dtype=np.uint8)
    _check(lib().wpt_radiance_rays(n, r.ctypes.data, None if k is None else k.ctypes.data, sample, spp, type, 0,
                                   rgb.ctypes.data, status.ctypes.data))
    return rgb, status


POINTS_COSINE = 0  # WPT_POINTS_COSINE: cosine-weighted about the normal (irradiance = pi * rgb / spp)
POINTS_SPHERE = 1  # WPT_POINTS_SPHERE: uniform over the sphere (mean radiance = rgb / spp)


def radiance_points(points, keys=None, sample=0, spp=1, type=1, dist=POINTS_COSINE, device=False):
    """Hemisphere gathers at a caller's points (wpt_radiance_points): record i =
    points[i] = {position, normal}; sample s of it leaves the point along a
    direction drawn on the device about the normal (dist: POINTS_COSINE or
    POINTS_SPHERE) and is then radiance_rays' path of that ray. Returns (rgb
    (n, 3) f32: the sum over the record's samples in sample order, status (n,)
    u8: 0 for a record with a non-finite component or a zero normal). keys,
    device and the session: as radiance_rays."""
    if device:
        import torch

        if points.dtype != torch.float32 or not points.is_contiguous() or points.numel() % 6:
            raise ValueError("points: a contiguous float32 tensor of 6 components per record")
        n = points.numel() // 6
        if keys is not None and (keys.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                                 or not keys.is_contiguous()
                                 or keys.numel() != n or keys.device != points.device):
            raise ValueError("keys: a contiguous 32-bit integer tensor of one key per record, on the points' device")
        rgb = torch.empty((n, 3), dtype=torch.float32, device=points.device)
        status = torch.empty((n,), dtype=torch.uint8, device=points.device)
        _check(lib().wpt_radiance_points(n, points.data_ptr(), keys.data_ptr() if keys is not None else None, sample,
                                         spp, type, dist, RAYS_DEVICE, rgb.data_ptr(), status.data_ptr()))
        return rgb, status
    r = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
    n = r.shape[0]
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint32).reshape(n)
    rgb = np.empty((n, 3), dtype=np.float32)
    status = np.empty(n, dtype=np.uint8)
    _check(lib().wpt_radiance_points(n, r.ctypes.data, None if k is None else k.ctypes.data, sample, spp, type, dist, 0,
                                     rgb.ctypes.data, status.ctypes.data))
    return rgb, status


def point_rays(points, keys=None, seed=0xBABABEBE, sample=0, dist=POINTS_COSINE):
    """The ray radiance_points makes for sample `sample` of every record
    (wpt_point_rays; host only, no session): (n, 6) f32 {origin, direction}, six
    +0 for an invalid record."""
    r = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
    n = r.shape[0]
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint32).reshape(n)
    rays = np.empty((n, 6), dtype=np.float32)
    _check(lib().wpt_point_rays(n, r.ctypes.data, None if k is None else k.ctypes.data, seed, sample, dist,
                                rays.ctypes.data))
    return rays


SH_MAX_ORDER = 2  # WPT_SH_MAX_ORDER
SH_CHUNK = 1 << 18  # WPT_SH_CHUNK: the records one internal pass of probe_sh takes (no result depends on it)


def probe_sh(points, keys=None, sample=0, spp=1, type=1, dist=POINTS_SPHERE, order=SH_MAX_ORDER, device=False):
    """Spherical-harmonic projection of a point's gathers (wpt_probe_sh):
    radiance_points' samples, each weighted by the real SH basis (sh_basis) of
    its own direction. Returns (sh (n, (order + 1)^2, 3) f32: per coefficient
    the sum over the record's traced samples in sample order, status (n,) u8 as
    radiance_points gives it). 4 pi / spp * sh (POINTS_SPHERE) estimates the
    radiance's SH coefficients. keys, device and the session: as radiance_rays."""
    nc = (order + 1) ** 2 if 0 <= order <= SH_MAX_ORDER else 1  # (the call rejects the order)
    if device:
        import torch

        if points.dtype != torch.float32 or not points.is_contiguous() or points.numel() % 6:
            raise ValueError("points: a contiguous float32 tensor of 6 components per record")
        n = points.numel() // 6
        if keys is not None and (keys.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                                 or not keys.is_contiguous()
                                 or keys.numel() != n or keys.device != points.device):
            raise ValueError("keys: a contiguous 32-bit integer tensor of one key per record, on the points' device")
        sh = torch.empty((n, nc, 3), dtype=torch.float32, device=points.device)
        status = torch.empty((n,), dtype=torch.uint8, device=points.device)
        _check(lib().wpt_probe_sh(n, points.data_ptr(), keys.data_ptr() if keys is not None else None, sample, spp,
                                  type, dist, order, RAYS_DEVICE, sh.data_ptr(), status.data_ptr()))
        return sh, status
    r = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
    n = r.shape[0]
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint32).reshape(n)
    sh = np.empty((n, nc, 3), dtype=np.float32)
    status = np.empty(n, dtype=np.uint8)
    _check(lib().wpt_probe_sh(n, r.ctypes.data, None if k is None else k.ctypes.data, sample, spp, type, dist, order, 0,
                              sh.ctypes.data, status.ctypes.data))
    return sh, status


def sh_basis(dirs, order=SH_MAX_ORDER):
    """The real SH basis probe_sh weights a sample with (wpt_sh_basis; host only,
    no session): (n, (order + 1)^2) f32 for directions (n, 3), used as given.
    World axes, z the polar axis, no Condon-Shortley sign."""
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    n = d.shape[0]
    out = np.empty((n, (order + 1) ** 2 if 0 <= order <= SH_MAX_ORDER else 1), dtype=np.float32)
    _check(lib().wpt_sh_basis(n, d.ctypes.data, order, out.ctypes.data))
    return out


def rays_valid(rays):
    """The status radiance_rays gives each ray (wpt_rays_valid; host only, no
    session): 1 if its six components are finite and its direction is not three
    zeros."""
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    status = np.empty(r.shape[0], dtype=np.uint8)
    _check(lib().wpt_rays_valid(r.shape[0], r.ctypes.data, status.ctypes.data))
    return status


FIRST_HIT_RAYS_PLANES = {  # name -> (argument position in wpt_first_hit_rays' outputs, dtype, components)
    "t": (0, np.float32, 1), "id": (1, np.int32, 1), "visits": (2, np.uint32, 1), "normal": (3, np.float32, 3),
    "albedo": (4, np.float32, 3), "kind": (5, np.uint8, 1), "status": (6, np.uint8, 1),
}


def _device_rays(rays):
    import torch

    if rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 6:
        raise ValueError("rays: a contiguous float32 tensor of 6 components per ray")
    return torch, rays.numel() // 6


def first_hit_rays(rays, planes=("t", "id", "visits", "normal", "albedo", "kind", "status"), device=False):
    """First-hit feature planes along a caller's rays (wpt_first_hit_rays): a
    dict plane name -> (n,) or (n, 3) array of the planes asked for, entry i
    what first_hit() gives a pixel whose primary ray is rays[i]; `status` is
    rays_valid()'s byte, and a ray of status 0 gets the miss entries with visits
    0. device=True: rays is a contiguous float32 torch tensor on the session's
    device, and so are the planes (id as torch.int32, visits as the bits of a
    torch.int32). The session is not touched."""
    out, ptr = {}, [None] * 7
    if device:
        torch, n = _device_rays(rays)
        tdt = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32, np.uint8: torch.uint8}
        for name in planes:
            pos, dt, c = FIRST_HIT_RAYS_PLANES[name]
            out[name] = torch.empty((n, 3) if c == 3 else (n,), dtype=tdt[dt], device=rays.device)
            ptr[pos] = out[name].data_ptr()
        _check(lib().wpt_first_hit_rays(n, rays.data_ptr(), RAYS_DEVICE, *ptr))
        return out
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = r.shape[0]
    for name in planes:
        pos, dt, c = FIRST_HIT_RAYS_PLANES[name]
        out[name] = np.empty((n, 3) if c == 3 else (n,), dtype=dt)
        ptr[pos] = out[name].ctypes.data
    _check(lib().wpt_first_hit_rays(n, r.ctypes.data, 0, *ptr))
    return out


DENOISE_ALBEDO = 1  # WPT_DENOISE_ALBEDO: filter radiance / albedo on diffuse hits, multiply the albedo back
# the documented defaults of denoise(): see profiles/denoise/README.md
DENOISE_DEFAULTS = {"iterations": 3, "sigma_c": 1.0, "sigma_z": 0.1, "flags": DENOISE_ALBEDO}


def _denoise_out(w, h):
    rgb = np.empty((h, w, 3), dtype=np.float32)
    valid = np.empty((h, w), dtype=np.uint8)
    rgba = np.empty((h, w, 4), dtype=np.uint8)
    return rgb, valid, rgba


def denoise(sample=0, iterations=DENOISE_DEFAULTS["iterations"], sigma_c=DENOISE_DEFAULTS["sigma_c"],
            sigma_z=DENOISE_DEFAULTS["sigma_z"], flags=DENOISE_DEFAULTS["flags"]):
    """The session's frame through the edge-avoiding a-trous filter
    (wpt_denoise), guided by the first-hit planes of sample `sample`:
    (rgb (H, W, 3) f32, valid (H, W) u8, rgba (H, W, 4) u8). Defaults: 3
    iterations (steps 1, 2, 4), sigma_c 1.0 (halved per iteration), sigma_z 0.1,
    albedo demodulation on. The session is not touched."""
    vp = get_option("viewport")
    rgb, valid, rgba = _denoise_out(vp & 0xFFFFFFFF, vp >> 32)
    _check(lib().wpt_denoise(sample, iterations, sigma_c, sigma_z, flags, rgb.ctypes.data, valid.ctypes.data,
                             rgba.ctypes.data))
    return rgb, valid, rgba


def _denoise_planes(fn, acc, cnt, t, normal, albedo, kind, iterations, sigma_c, sigma_z, flags):
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    h, w = cnt.shape
    acc = np.ascontiguousarray(acc, dtype=np.float32).reshape(h, w, 3)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(h, w)
    normal = np.ascontiguousarray(normal, dtype=np.float32).reshape(h, w, 3)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32).reshape(h, w, 3)
    kind = np.ascontiguousarray(kind, dtype=np.uint8).reshape(h, w)
    rgb, valid, rgba = _denoise_out(w, h)
    _check(fn(w, h, acc.ctypes.data, cnt.ctypes.data, t.ctypes.data, normal.ctypes.data, albedo.ctypes.data,
              kind.ctypes.data, iterations, sigma_c, sigma_z, flags, rgb.ctypes.data, valid.ctypes.data,
              rgba.ctypes.data))
    return rgb, valid, rgba


def denoise_planes(acc, cnt, t, normal, albedo, kind, iterations=DENOISE_DEFAULTS["iterations"],
                   sigma_c=DENOISE_DEFAULTS["sigma_c"], sigma_z=DENOISE_DEFAULTS["sigma_z"],
                   flags=DENOISE_DEFAULTS["flags"]):
    """Test hook (wpt_denoise_planes): denoise()'s kernels on the caller's
    planes; cnt is (H, W) and sizes the frame. Needs init."""
    return _denoise_planes(lib().wpt_denoise_planes, acc, cnt, t, normal, albedo, kind, iterations, sigma_c, sigma_z,
                           flags)


def denoise_host(acc, cnt, t, normal, albedo, kind, iterations=DENOISE_DEFAULTS["iterations"],
                 sigma_c=DENOISE_DEFAULTS["sigma_c"], sigma_z=DENOISE_DEFAULTS["sigma_z"],
                 flags=DENOISE_DEFAULTS["flags"]):
    """The filter's host restatement (wpt_denoise_host): no session, no GPU."""
    return _denoise_planes(lib().wpt_denoise_host, acc, cnt, t, normal, albedo, kind, iterations, sigma_c, sigma_z,
                           flags)


DENOISE_RAYS_OUTPUTS = {  # name -> (argument position in wpt_denoise_rays' outputs, dtype, components)
    "rgb": (0, np.float32, 3), "valid": (1, np.uint8, 1), "rgba": (2, np.uint8, 4), "raw": (3, np.float32, 3),
    "status": (4, np.uint8, 1),
}


def denoise_rays(rays, width, height, keys=None, sample=0, spp=1, type=1,
                 iterations=DENOISE_DEFAULTS["iterations"], sigma_c=DENOISE_DEFAULTS["sigma_c"],
                 sigma_z=DENOISE_DEFAULTS["sigma_z"], flags=DENOISE_DEFAULTS["flags"],
                 outputs=("rgb", "valid", "rgba", "raw", "status"), device=False):
    """A filtered width x height frame along a caller's rays (wpt_denoise_rays):
    rays[y * width + x] is pixel (x, y). A dict of the outputs asked for: `raw`
    (H, W, 3) f32 and `status` (H, W) u8 are radiance_rays(rays, keys, sample,
    spp, type); `rgb` (H, W, 3) f32, `valid` (H, W) u8 and `rgba` (H, W, 4) u8
    are denoise_host() of raw, cnt = spp * status and first_hit_rays()' guide
    planes of the same rays, all kept on the device. `flags` are the filter's
    (DENOISE_ALBEDO). device=True: rays (and keys) are contiguous torch tensors
    on the session's device, and so are the outputs."""
    n = width * height
    out, ptr = {}, [None] * 5
    if device:
        torch, nr = _device_rays(rays)
        if nr != n:
            raise ValueError("rays: width * height rays")
        if keys is not None and (keys.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                                 or not keys.is_contiguous() or keys.numel() != n or keys.device != rays.device):
            raise ValueError("keys: a contiguous 32-bit integer tensor of one key per ray, on the rays' device")
        for name in outputs:
            pos, dt, c = DENOISE_RAYS_OUTPUTS[name]
            out[name] = torch.empty((height, width) if c == 1 else (height, width, c),
                                    dtype=torch.float32 if dt is np.float32 else torch.uint8, device=rays.device)
            ptr[pos] = out[name].data_ptr()
        _check(lib().wpt_denoise_rays(width, height, rays.data_ptr(), keys.data_ptr() if keys is not None else None,
                                      sample, spp, type, iterations, sigma_c, sigma_z, flags, RAYS_DEVICE, *ptr))
        return out
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    if r.shape[0] != n:
        raise ValueError("rays: width * height rays")
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint32).reshape(n)
    for name in outputs:
        pos, dt, c = DENOISE_RAYS_OUTPUTS[name]
        out[name] = np.empty((height, width) if c == 1 else (height, width, c), dtype=dt)
        ptr[pos] = out[name].ctypes.data
    _check(lib().wpt_denoise_rays(width, height, r.ctypes.data, None if k is None else k.ctypes.data, sample, spp, type,
                                  iterations, sigma_c, sigma_z, flags, 0, *ptr))
    return out


REPROJECT_KEEP, REPROJECT_NEAREST, REPROJECT_SAME_SHAPE = 1, 2, 4  # WPT_REPROJECT_*
# the documented defaults of reproject(): see profiles/reproject/README.md
REPROJECT_DEFAULTS = {"cos_min": 0.9, "eps_z": 0.05, "max_len": 64, "flags": 0}


def reproject(sample=0, cos_min=REPROJECT_DEFAULTS["cos_min"], eps_z=REPROJECT_DEFAULTS["eps_z"],
              max_len=REPROJECT_DEFAULTS["max_len"], flags=REPROJECT_DEFAULTS["flags"]):
    """The session's frame merged with the kept history reprojected into the
    current camera (wpt_reproject), through the first-hit planes of sample
    `sample`: (acc (H, W, 3) f32, cnt (H, W) u32, len (H, W) u32). With
    REPROJECT_KEEP the merged frame becomes the history: call it once, right
    before update_camera. Without it nothing of the session changes."""
    vp = get_option("viewport")
    w, h = vp & 0xFFFFFFFF, vp >> 32
    acc = np.empty((h, w, 3), dtype=np.float32)
    cnt = np.empty((h, w), dtype=np.uint32)
    ln = np.empty((h, w), dtype=np.uint32)
    _check(lib().wpt_reproject(sample, cos_min, eps_z, max_len, flags, acc.ctypes.data, cnt.ctypes.data,
                               ln.ctypes.data))
    return acc, cnt, ln


def history_drop():
    """Forget reproject()'s kept history (wpt_history_drop)."""
    _check(lib().wpt_history_drop())


def denoise_merged(iterations=DENOISE_DEFAULTS["iterations"], sigma_c=DENOISE_DEFAULTS["sigma_c"],
                   sigma_z=DENOISE_DEFAULTS["sigma_z"], flags=DENOISE_DEFAULTS["flags"]):
    """denoise()'s filter over the merged frame and guide planes the last
    reproject() left on the device (wpt_denoise_merged): (rgb, valid, rgba)."""
    vp = get_option("viewport")
    rgb, valid, rgba = _denoise_out(vp & 0xFFFFFFFF, vp >> 32)
    _check(lib().wpt_denoise_merged(iterations, sigma_c, sigma_z, flags, rgb.ctypes.data, valid.ctypes.data,
                                    rgba.ctypes.data))
    return rgb, valid, rgba


def _reproject_planes(fn, cam, cur, prev_cam, hist, cos_min, eps_z, max_len, flags):
    acc, cnt, dirs, t, ids, normal, kind = cur
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    h, w = cnt.shape

    def f3(a):
        return np.ascontiguousarray(a, dtype=np.float32).reshape(h, w, 3)

    def p1(a, dt):
        return np.ascontiguousarray(a, dtype=dt).reshape(h, w)

    h_acc, h_cnt, h_t, h_id, h_normal, h_kind = hist
    ins = [np.ascontiguousarray(cam, dtype=np.float32).reshape(-1)[:3].copy(), f3(acc), cnt, f3(dirs),
           p1(t, np.float32), p1(ids, np.int32), f3(normal), p1(kind, np.uint8),
           np.ascontiguousarray(prev_cam, dtype=np.float32).reshape(5), f3(h_acc), p1(h_cnt, np.uint32),
           p1(h_t, np.float32), p1(h_id, np.int32), f3(h_normal), p1(h_kind, np.uint8)]
    acc_o = np.empty((h, w, 3), dtype=np.float32)
    cnt_o = np.empty((h, w), dtype=np.uint32)
    len_o = np.empty((h, w), dtype=np.uint32)
    _check(fn(w, h, *[a.ctypes.data for a in ins], cos_min, eps_z, max_len, flags, acc_o.ctypes.data,
              cnt_o.ctypes.data, len_o.ctypes.data))
    return acc_o, cnt_o, len_o


def reproject_planes(cam, cur, prev_cam, hist, cos_min=REPROJECT_DEFAULTS["cos_min"],
                     eps_z=REPROJECT_DEFAULTS["eps_z"], max_len=REPROJECT_DEFAULTS["max_len"],
                     flags=REPROJECT_DEFAULTS["flags"]):
    """Test hook (wpt_reproject_planes): reproject()'s kernel on the caller's
    planes. cam: the current camera (its position is used); cur = (acc, cnt, dir,
    t, id, normal, kind), cnt (H, W) sizing the frame; prev_cam = (x, y, z, rot_x,
    rot_y) and hist = (acc, cnt, t, id, normal, kind): the history. Needs init."""
    return _reproject_planes(lib().wpt_reproject_planes, cam, cur, prev_cam, hist, cos_min, eps_z, max_len, flags)


def reproject_host(cam, cur, prev_cam, hist, cos_min=REPROJECT_DEFAULTS["cos_min"],
                   eps_z=REPROJECT_DEFAULTS["eps_z"], max_len=REPROJECT_DEFAULTS["max_len"],
                   flags=REPROJECT_DEFAULTS["flags"]):
    """Reprojection's host restatement (wpt_reproject_host): no session, no GPU."""
    return _reproject_planes(lib().wpt_reproject_host, cam, cur, prev_cam, hist, cos_min, eps_z, max_len, flags)


def first_hit_scaled(scale, sample=0, planes=("dir", "t", "id", "visits", "normal", "albedo", "kind")):
    """first_hit()'s planes for the virtual viewport scale * W x scale * H under
    the session's camera and seed (wpt_first_hit_scaled): a dict plane name ->
    (scale * H, scale * W) or (scale * H, scale * W, 3) array. scale 1..4."""
    vp = get_option("viewport")
    w, h = scale * (vp & 0xFFFFFFFF), scale * (vp >> 32)
    out, ptr = {}, [None] * 7
    for name in planes:
        pos, dt, c = FIRST_HIT_PLANES[name]
        out[name] = np.empty((h, w, 3) if c == 3 else (h, w), dtype=dt)
        ptr[pos] = out[name].ctypes.data
    _check(lib().wpt_first_hit_scaled(scale, sample, *ptr))
    return out


UPSAMPLE_MERGED = 1  # WPT_UPSAMPLE_MERGED: the source is the last reproject()'s merged frame and guides
# the documented defaults of upsample(): the filter's sigmas and passes (profiles/upsample/README.md)
UPSAMPLE_DEFAULTS = {"scale": 2, "iterations": DENOISE_DEFAULTS["iterations"], "sigma_c": DENOISE_DEFAULTS["sigma_c"],
                     "sigma_z": DENOISE_DEFAULTS["sigma_z"], "flags": 0}


def upsample(scale=UPSAMPLE_DEFAULTS["scale"], sample=0, iterations=UPSAMPLE_DEFAULTS["iterations"],
             sigma_c=UPSAMPLE_DEFAULTS["sigma_c"], sigma_z=UPSAMPLE_DEFAULTS["sigma_z"],
             flags=UPSAMPLE_DEFAULTS["flags"]):
    """The session's W x H frame upsampled to scale * W x scale * H under
    first-hit planes made at the fine viewport (wpt_upsample): (rgb (sH, sW, 3)
    f32, valid (sH, sW) u8: 0 nothing passed, 1 exact or the four taps, 2 the
    4 x 4 block, rgba (sH, sW, 4) u8). iterations 0..5 of the filter run on the
    coarse irradiance first. With UPSAMPLE_MERGED the source is the last
    reproject()'s merged frame. The session is not touched."""
    vp = get_option("viewport")
    rgb, valid, rgba = _denoise_out(scale * (vp & 0xFFFFFFFF), scale * (vp >> 32))
    _check(lib().wpt_upsample(scale, sample, iterations, sigma_c, sigma_z, flags, rgb.ctypes.data, valid.ctypes.data,
                              rgba.ctypes.data))
    return rgb, valid, rgba


def _upsample_planes(fn, scale, coarse, fine, background, iterations, sigma_c, sigma_z, flags):
    acc, cnt, t, normal, albedo, kind = coarse
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    h, w = cnt.shape
    fh, fw = scale * h, scale * w
    acc = np.ascontiguousarray(acc, dtype=np.float32).reshape(h, w, 3)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(h, w)
    normal = np.ascontiguousarray(normal, dtype=np.float32).reshape(h, w, 3)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32).reshape(h, w, 3)
    kind = np.ascontiguousarray(kind, dtype=np.uint8).reshape(h, w)
    ht, hn, ha, hk = fine
    ht = np.ascontiguousarray(ht, dtype=np.float32).reshape(fh, fw)
    hn = np.ascontiguousarray(hn, dtype=np.float32).reshape(fh, fw, 3)
    ha = np.ascontiguousarray(ha, dtype=np.float32).reshape(fh, fw, 3)
    hk = np.ascontiguousarray(hk, dtype=np.uint8).reshape(fh, fw)
    bg = np.ascontiguousarray(background, dtype=np.float32).reshape(3)
    rgb, valid, rgba = _denoise_out(fw, fh)
    _check(fn(w, h, scale, acc.ctypes.data, cnt.ctypes.data, t.ctypes.data, normal.ctypes.data, albedo.ctypes.data,
              kind.ctypes.data, ht.ctypes.data, hn.ctypes.data, ha.ctypes.data, hk.ctypes.data, bg.ctypes.data,
              iterations, sigma_c, sigma_z, flags, rgb.ctypes.data, valid.ctypes.data, rgba.ctypes.data))
    return rgb, valid, rgba


def upsample_planes(scale, coarse, fine, background=(0.0, 0.0, 0.0), iterations=UPSAMPLE_DEFAULTS["iterations"],
                    sigma_c=UPSAMPLE_DEFAULTS["sigma_c"], sigma_z=UPSAMPLE_DEFAULTS["sigma_z"], flags=0):
    """Test hook (wpt_upsample_planes): upsample()'s kernels on the caller's
    planes. coarse = (acc, cnt, t, normal, albedo, kind) at (H, W), cnt sizing
    the frame; fine = (t, normal, albedo, kind) at (scale * H, scale * W).
    Needs init."""
    return _upsample_planes(lib().wpt_upsample_planes, scale, coarse, fine, background, iterations, sigma_c, sigma_z,
                            flags)


def upsample_host(scale, coarse, fine, background=(0.0, 0.0, 0.0), iterations=UPSAMPLE_DEFAULTS["iterations"],
                  sigma_c=UPSAMPLE_DEFAULTS["sigma_c"], sigma_z=UPSAMPLE_DEFAULTS["sigma_z"], flags=0):
    """The upsampler's host restatement (wpt_upsample_host): no session, no GPU."""
    return _upsample_planes(lib().wpt_upsample_host, scale, coarse, fine, background, iterations, sigma_c, sigma_z,
                            flags)


MAP_MISS_ONCE = 1  # WPT_MAP_MISS_ONCE: a pixel whose ray of `sample` misses needs one sample only


def sample_map(sample=0, target=8, max_per_pixel=8, budget=0, flags=0):
    """A sample map planned from the session's counts and the history length
    the last reproject() of this accumulation recovered (wpt_sample_map):
    (count (H, W) u32, (T, dealt)). A pixel needs min(target - min(cnt + len,
    2^32 - 1), max_per_pixel) samples (0 outside the partition); T is the sum
    of the needs; budget 0 or >= T gives every pixel its need, a smaller one is
    dealt in proportion, exactly. The map stays on the device for
    compute_map(None); the session is not touched."""
    vp = get_option("viewport")
    w, h = vp & 0xFFFFFFFF, vp >> 32
    count = np.empty((h, w), dtype=np.uint32)
    tot = np.zeros(2, dtype=np.uint64)
    _check(lib().wpt_sample_map(sample, target, max_per_pixel, budget, flags, count.ctypes.data, tot.ctypes.data))
    return count, (int(tot[0]), int(tot[1]))


def compute_map(count=None):
    """Traces a sample map (wpt_compute_map): pixel p of this rank's partition
    gets count[p] samples starting at its sample count. None: the map the last
    sample_map() of this accumulation left on the device. Once a map traced a
    sample, compute() is an error until the accumulation is reset
    (get_option("map_mode") reads 1)."""
    if count is None:
        _check(lib().wpt_compute_map(None))
        return
    vp = get_option("viewport")
    w, h = vp & 0xFFFFFFFF, vp >> 32
    c = np.ascontiguousarray(count, dtype=np.uint32).reshape(h, w)
    _check(lib().wpt_compute_map(c.ctypes.data))


def _sample_map_planes(fn, cnt, length, kind, member, target, max_per_pixel, budget, flags):
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    h, w = cnt.shape
    length = np.ascontiguousarray(length, dtype=np.uint32).reshape(h, w)
    kind = np.ascontiguousarray(kind, dtype=np.uint8).reshape(h, w)
    member = np.ascontiguousarray(member, dtype=np.uint8).reshape(h, w)
    count = np.empty((h, w), dtype=np.uint32)
    tot = np.zeros(2, dtype=np.uint64)
    _check(fn(w, h, cnt.ctypes.data, length.ctypes.data, kind.ctypes.data, member.ctypes.data, target, max_per_pixel,
              budget, flags, count.ctypes.data, tot.ctypes.data))
    return count, (int(tot[0]), int(tot[1]))


def sample_map_planes(cnt, length, kind, member, target=8, max_per_pixel=8, budget=0, flags=0):
    """Test hook (wpt_sample_map_planes): sample_map()'s kernels on the caller's
    planes; cnt is (H, W) and sizes the frame, member is 1 for the pixels of the
    partition. Needs init."""
    return _sample_map_planes(lib().wpt_sample_map_planes, cnt, length, kind, member, target, max_per_pixel, budget,
                              flags)


def sample_map_host(cnt, length, kind, member, target=8, max_per_pixel=8, budget=0, flags=0):
    """The sample map's host restatement (wpt_sample_map_host): no session, no GPU."""
    return _sample_map_planes(lib().wpt_sample_map_host, cnt, length, kind, member, target, max_per_pixel, budget,
                              flags)


def presolve_rays(rays):
    """The producers' presolve on the device (wpt_presolve_rays): per ray
    (resolved, t, id); (t, id) is the closest hit of a resolved ray."""
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = r.shape[0]
    res = np.zeros(n, dtype=np.uint8)
    t = np.empty(n, dtype=np.float32)
    ids = np.empty(n, dtype=np.int32)
    _check(lib().wpt_presolve_rays(n, r.ctypes.data, res.ctypes.data, t.ctypes.data, ids.ctypes.data))
    return res.astype(bool), t, ids


def presolve_shadow_rays(pq, light_ids):
    """k_shade's presolve of shadow rays on the device
    (wpt_presolve_shadow_rays): per {p, q} pair and light shape id, whether
    the ray provably ends unoccluded."""
    p = np.ascontiguousarray(pq, dtype=np.float32).reshape(-1, 6)
    li = np.ascontiguousarray(light_ids, dtype=np.int32)
    res = np.zeros(p.shape[0], dtype=np.uint8)
    _check(lib().wpt_presolve_shadow_rays(p.shape[0], p.ctypes.data, li.ctypes.data, res.ctypes.data))
    return res.astype(bool)


def shutdown():
    _check(lib().wpt_shutdown())


class DebugScene:
    """View of a scene as wpt_init would build it: BVH2 built on the host (no
    GPU), or with gpu=True by the GPU build (wpt_debug_scene_new_gpu)."""

    def __init__(self, scene_id, mesh=None, gpu=False):
        L = lib()
        m = None if mesh is None else np.ascontiguousarray(mesh, dtype=np.float32)
        new = L.wpt_debug_scene_new_gpu if gpu else L.wpt_debug_scene_new
        self.h = new(scene_id, None if m is None else m.ctypes.data, 0 if m is None else m.size // 3)
        if not self.h:
            raise WptError(ERR_INVALID_SCENE, L.wpt_last_error().decode())
        bi = np.zeros(2, dtype=np.float64)
        _check(L.wpt_debug_scene_build_info(self.h, bi.ctypes.data))
        self.bvh_ms, self.bvh_on_gpu = float(bi[0]), bool(bi[1])
        info = np.zeros(8, dtype=np.uint64)
        L.wpt_debug_scene_info(self.h, info.ctypes.data)
        (self.num_shapes, self.num_inf, self.num_nodes, self.num_lights, self.depth, self.use_bvh,
         self.tri_only, self.num_nodes4) = (int(x) for x in info)

    def nodes(self):
        out = np.empty((self.num_nodes, 8), dtype=np.uint32)
        lib().wpt_debug_scene_nodes(self.h, out.ctypes.data)
        return out

    def nodes4(self):
        """The BVH4: (nodes, 37) u32 rows (include/wpt.h wpt_debug_scene_nodes4)."""
        out = np.empty((self.num_nodes4, 37), dtype=np.uint32)
        if self.num_nodes4:
            lib().wpt_debug_scene_nodes4(self.h, out.ctypes.data)
        return out

    def shapes(self):
        out = np.empty((self.num_shapes, 16), dtype=np.float32)
        lib().wpt_debug_scene_shapes(self.h, out.ctypes.data)
        return out

    def materials(self):
        """(shapes, 4) f32: Diffuse colour or Emissive intensity, 1 if emissive."""
        out = np.empty((self.num_shapes, 4), dtype=np.float32)
        _check(lib().wpt_debug_scene_materials(self.h, out.ctypes.data))
        return out

    def lights(self):
        out = np.empty(self.num_lights, dtype=np.uint32)
        lib().wpt_debug_scene_lights(self.h, out.ctypes.data)
        return out

    def presolve(self, rays):
        """The presolve's host restatement (as presolve_rays, no GPU)."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = r.shape[0]
        res = np.zeros(n, dtype=np.uint8)
        t = np.empty(n, dtype=np.float32)
        ids = np.empty(n, dtype=np.int32)
        _check(lib().wpt_debug_scene_presolve(self.h, n, r.ctypes.data, res.ctypes.data, t.ctypes.data,
                                              ids.ctypes.data))
        return res.astype(bool), t, ids

    def presolve_shadow(self, pq, light_ids):
        """The shadow presolve's host restatement (as presolve_shadow_rays, no GPU)."""
        p = np.ascontiguousarray(pq, dtype=np.float32).reshape(-1, 6)
        li = np.ascontiguousarray(light_ids, dtype=np.int32)
        res = np.zeros(p.shape[0], dtype=np.uint8)
        _check(lib().wpt_debug_scene_presolve_shadow(self.h, p.shape[0], p.ctypes.data, li.ctypes.data,
                                                     res.ctypes.data))
        return res.astype(bool)

    def guard_lights(self):
        """(bit mask of the light guards, shape ids of their primitives)."""
        m, n = ctypes.c_uint32(0), ctypes.c_uint32(0)
        ids = np.full(4, -1, dtype=np.int32)
        _check(lib().wpt_debug_scene_guard_lights(self.h, ctypes.addressof(m), ctypes.addressof(n), ids.ctypes.data))
        return m.value, ids[: n.value].copy()

    def guards(self):
        """(root box (6,), guard boxes (n, 6), per-node guard of a leaf or 0xFFFFFFFF)."""
        ng = ctypes.c_uint32(0)
        boxes = np.zeros(30, dtype=np.float32)
        lg = np.zeros(max(self.num_nodes, 1), dtype=np.uint32)
        _check(lib().wpt_debug_scene_guards(self.h, ctypes.addressof(ng), boxes.ctypes.data, lg.ctypes.data))
        return boxes[:6].copy(), boxes[6:].reshape(4, 6)[: ng.value].copy(), lg[: self.num_nodes]

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().wpt_debug_scene_free(self.h)
                self.h = None
        except Exception:
            pass
