/*
 * wpt.h — C ABI of the MI355X path-tracing core (libwpt.so).
 *
 * Drop-in boundary for sourcedennis/wasm-pathtracer's `src/wasm_interface.rs`
 * (the only FFI surface of the reference: primitive-only `#[wasm_bindgen]`
 * free functions over one global session). Each `wpt_<name>` below replaces
 * the reference export `<name>` cited next to it, with the same argument
 * meaning. Where the reference `panic!`s (a WASM trap) these functions return
 * a negative WPT_ERR_* status instead; wpt_last_error() gives the message.
 * Pointers returned to the caller stay owned by the library, valid until the
 * next init / viewport / scene / mesh change, as in the reference.
 *
 * Additions (no reference counterpart) are grouped at the end: render
 * options (depth cap, seed), multi-GPU pixel partition, f32 radiance access
 * for parity, statistics and kernel timings.
 *
 * Threading: like the reference (Rc/RefCell, one instance per worker) the
 * session is single-threaded; call from one host thread per process.
 */
#ifndef WPT_H
#define WPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (the reference panics instead) */
#define WPT_OK 0
#define WPT_ERR_NOT_INIT (-1)      /* "init not called"      wasm_interface.rs:131 */
#define WPT_ERR_ALREADY_INIT (-2)  /* "Cannot init again"    wasm_interface.rs:75  */
#define WPT_ERR_INVALID_SCENE (-3) /* "Invalid scene"        wasm_interface.rs:396 */
#define WPT_ERR_INVALID_ARG (-4)   /* "Invalid RenderType magic number" :212, bad sizes */
#define WPT_ERR_UNSUPPORTED (-5)   /* feature not in this core (e.g. a scene whose build is unsupported) */
#define WPT_ERR_DEVICE (-6)        /* HIP runtime error */
#define WPT_ERR_NO_MESH (-7)       /* "Mesh not allocated"   wasm_interface.rs:281 */

/* render types (wasm_interface.rs:207-214) */
#define WPT_NO_NEE 0
#define WPT_NORMAL_NEE 1
#define WPT_PNEE 2

/* ---- reference exports (src/wasm_interface.rs) ------------------------- */

/* init(width, height, scene_id, cam_x, cam_y, cam_z, cam_rot_x, cam_rot_y)
 * wasm_interface.rs:67-113. Scene ids: 0 = museum (scenes.rs:15-68), 2 = bunny
 * scene (mesh slot 1), plus the build-defined configs 100 (C1 box) and 101 (C2
 * spheres, BVH disabled). Initial settings as the reference's (:90-94): left
 * half NormalNEE with random sampling, right half PNEE with adaptive
 * sampling; the sampling view starts blue. */
int wpt_init(uint32_t width, uint32_t height, uint32_t scene_id, float cam_x, float cam_y, float cam_z,
             float cam_rot_x, float cam_rot_y);

/* results(is_show_sampling) -> *const u8 — wasm_interface.rs:120-134.
 * RGBA8, width*height*4 bytes, re-quantised as render_target.rs:62-64.
 * is_show_sampling = 1: the sampling view (SimpleRenderTarget). Every reset
 * (settings, viewport, camera, scene, render options) clears it to black and
 * the adaptive halves repaint themselves blue, as reset() / update_scene() /
 * update_settings() do in the reference (wasm_interface.rs:137-201). */
const uint8_t* wpt_results(uint32_t is_show_sampling);

/* update_scene(scene_id) — wasm_interface.rs:154-169 */
int wpt_update_scene(uint32_t scene_id);

/* update_settings(left_type, right_type, is_left_adaptive, is_right_adaptive,
 * is_light_debug) — wasm_interface.rs:173-204 */
int wpt_update_settings(uint32_t left_type, uint32_t right_type, uint32_t is_left_adaptive,
                        uint32_t is_right_adaptive, uint32_t is_light_debug);

/* update_viewport(width, height) — wasm_interface.rs:219-232 */
int wpt_update_viewport(uint32_t width, uint32_t height);

/* update_camera(x, y, z, rot_x, rot_y) — wasm_interface.rs:239-248 */
int wpt_update_camera(float cam_x, float cam_y, float cam_z, float cam_rot_x, float cam_rot_y);

/* allocate_mesh(id, num_vertices) — wasm_interface.rs:259-270 */
int wpt_allocate_mesh(uint32_t id, uint32_t num_vertices);

/* mesh_vertices(id) -> *mut Vec3 — wasm_interface.rs:275-287.
 * Packed f32 x,y,z per vertex, filled by the caller. NULL if not allocated. */
float* wpt_mesh_vertices(uint32_t id);

/* notify_mesh_loaded(id) -> bool — wasm_interface.rs:293-329.
 * Returns 1 if the active scene uses the mesh and was rebuilt, 0 if not. */
int wpt_notify_mesh_loaded(uint32_t id);
/* Mesh ingestion (the reference client's side of allocate_mesh /
 * mesh_vertices): parses OBJ text as src_ts/client/obj_parser.ts:3-51 does
 * (wasm-pathtracer_amd/csrc/wpt_obj.h: 'v' and triangular 'f' only, fields
 * split on single spaces, JavaScript parseFloat / parseInt) into mesh slot
 * `id` as a triangle soup, then scales it per axis if `scale` is non-null
 * (index.ts:216-220 uses (8, 8, -8) for the bunny). *num_vertices = 3 per
 * face. Call wpt_notify_mesh_loaded(id) next, as after mesh_vertices.
 * WPT_ERR_INVALID_ARG on a non-triangular face (the reference throws). */
int wpt_load_obj(uint32_t id, const char* text, size_t len, const float* scale, uint64_t* num_vertices);
/* The same parse without a session (host only): *num_vertices always; the
 * vertices (3 floats each) into `out` when it is non-null and holds
 * `capacity` vertices. */
int wpt_parse_obj(const char* text, size_t len, const float* scale, float* out, uint64_t capacity,
                  uint64_t* num_vertices);

/* allocate_texture(id, width, height) -> *mut (u8,u8,u8) — wasm_interface.rs:335-352 */
uint8_t* wpt_allocate_texture(uint32_t id, uint32_t width, uint32_t height);

/* notify_texture_loaded(id) -> bool (always false) — wasm_interface.rs:358-366 */
int wpt_notify_texture_loaded(uint32_t id);

/* compute(num_samples) — wasm_interface.rs:374-384 (RenderInstance::compute,
 * tracer.rs:103-123). Traces num_samples paths; pixels left of width/2 use
 * left_type, the others right_type.
 * As the reference (two RenderInstances, :377-379), each screen half has its
 * own sample sequence and gets n/2 (left) and n - n/2 (right) of the n
 * samples, on one rank whatever the strategies.
 * Deliberate differences (build-defined):
 *  - pixel order: a random half takes one sample per pixel per round in
 *    raster order (the reference picks pixels at random); whole rounds are
 *    traced in 8x8 tiles (the same (pixel, sample) pairs). An adaptive half
 *    takes AdaptiveSamplingStrategy's rounds (4 per pixel, then ceil(1 + 32
 *    scaled_mse)) in raster order instead of LIFO-shuffled order.
 *  - several ranks (wpt_set_partition / wpt_set_comm): with random halves
 *    compute(n) traces n paths over this rank's pixel list in partition order
 *    (path k -> pixel k mod P, sample k div P: per-GPU work fixed); with an
 *    adaptive half n positions of the GLOBAL per-half sequences (the same n
 *    on every rank).
 *  - RNG: each path has its own xorshift32 stream path_seed(seed, pixel,
 *    sample) with the reference's draw order inside the path.
 *  - PNEE: the 300000 photons are shot once, before the first path, on
 *    per-photon streams, and both halves share the one tree; the reference
 *    spends compute ticks on photons (32 per tick, tracer.rs:103-123) and
 *    builds one tree per half, so its first compute calls trace fewer paths. */
int wpt_compute(size_t num_samples);

/* ---- additions ---------------------------------------------------------- */

/* Last error message (thread-local to the session). */
const char* wpt_last_error(void);

/* Select the HIP device before wpt_init (default: 0). */
int wpt_set_device(int device);

/* Depth cap (0 = the reference's unbounded Russian-roulette loop), frame seed
 * for the per-path xorshift32 streams (default 0xBABABEBE, rng.rs:11) and the
 * number of paths resident per wavefront batch (0 = keep). Resets accumulation. */
int wpt_set_render_options(int32_t max_depth, uint32_t frame_seed, uint64_t batch_paths);

/* Multi-GPU partition: square tiles of `tile` px in raster order, tile t is
 * rendered by rank t % nranks; a rank's pixels are listed tile by tile, 8x8
 * sub-tiles in raster order inside a tile. Resets accumulation. */
int wpt_set_partition(uint32_t rank, uint32_t nranks, uint32_t tile);

/* Number of pixels of this rank's partition; fills `out` (may be NULL) with
 * their viewport indices (y*width+x) in partition order. */
int64_t wpt_partition_pixels(uint32_t* out);

/* Host-only (no session, no GPU): the pixel list wpt_set_partition would give
 * rank `rank` of `nranks` on a width x height viewport; returns its length. */
int64_t wpt_tile_partition(uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks, uint32_t tile,
                           uint32_t* out);

/* PNEE photon octree (photon_tree.rs), built on first use: shoots photons
 * k = 0,1,... on per-photon streams until 300000 are stored (tracer.rs:104),
 * inserts them in photon order, freezes the CDFs. Returns the node count;
 * fills (each may be NULL) child[node] (first of 8 children, 0 = leaf),
 * cum[node * num_lights + light] (cum_bins) and shot_stored[2]. */
int64_t wpt_photon_tree(uint32_t* child, float* cum, uint64_t* shot_stored);

/* Host-only (no session, no GPU): the frozen octree of a caller's photon list
 * (light id < num_lights, location xyz, intensity; inserted in this order).
 * Returns the node count; fills (each may be NULL: size query) child and cum
 * as wpt_photon_tree does, and corners[64 * node + 8 * case + c], the table of
 * the 8 cells of the device's trilinear mix per leaf and offset case (x, y, z
 * offset +1: bits 2, 1, 0 of the case; corner c: bit 2 x, bit 1 y, bit 0 z
 * shifted to the adjacent cell, clamped to the root box). Internal nodes and
 * leaves deeper than 20 levels have zero rows: the device finds their cells by
 * descents. WPT_ERR_INVALID_ARG for a light id out of range. */
int64_t wpt_photon_build(uint32_t num_lights, uint64_t n, const uint32_t* light, const float* loc3,
                         const float* intensity, uint32_t* child, float* cum, uint32_t* corners);

/* Test hook: the photon list as the session's PNEE octree, for the scene's
 * light count, frozen and uploaded as a shot tree is. It stays until what
 * drops a shot tree drops it (a new scene, a new frame seed); the session then
 * shoots its own again. WPT_ERR_INVALID_ARG for a light id >= the light
 * count. */
int wpt_install_photons(uint64_t n, const uint32_t* light, const float* loc3, const float* intensity);

/* Test hook: the device's PhotonTree::sample (photon_tree.rs:80-159) on the
 * session's octree, point i (points3[3 i ..]) on the xorshift32 state
 * states[i]: the light picked, its pdf and the state afterwards. view: where
 * the kernel reads the tree, as the shade kernel's three variants do (0 global
 * memory, 1 child array in LDS, 2 child array and CDFs in LDS);
 * WPT_ERR_INVALID_ARG if the tree does not fit it. table 0: the neighbour
 * cells by walks only, not from the corner table. */
int wpt_photon_sample(size_t n, const float* points3, const uint32_t* states, int32_t view, int32_t table,
                      uint32_t* light, float* pdf, uint32_t* states_out);

/* Accumulated radiance: acc3 = width*height*3 f32 (sum over samples, as
 * RenderTarget.acc_buffer), cnt = width*height u32 (acc_count). */
int wpt_read_radiance(float* acc3, uint32_t* cnt);

/* Device-to-device copy of this rank's partition as float4 (acc.xyz, count)
 * into `device_dst` (partition_pixels * 16 bytes, same device). */
int wpt_copy_partition(void* device_dst);

/* Adaptive sampling over several ranks. A round's error
 * estimate reads every pixel's radiance, including the 2-pixel halo of
 * gaussian5 (render_target.rs:112-128) across tile borders, so at each round
 * boundary the ranks exchange their partitions: the library packs its own
 * (float4 per partition pixel: acc.xyz, sample count as u32 bits) into
 * `local_dev` and calls fn(user), which must all-gather the `slot`-float4
 * buffers of all ranks, rank-major, into `gathered_dev` (nranks * slot float4,
 * same device), synchronised, and return 0 (non-zero aborts compute). Every
 * rank then plans the same global round over the whole frame.
 * With adaptive halves and several ranks, compute(n) advances the GLOBAL
 * round sequence by n positions (every rank passes the same n) and each rank
 * traces the positions on its own pixels; the union of the partitions is then
 * bitwise the single-rank frame after compute(n). With WPT_OPT_STOCK_RANKS a
 * rank takes those samples from the sample stock of its partition, traced
 * ahead of the rounds; the exchanges, one per round of an adaptive half after
 * its first, are the same calls in the same order on every rank either way,
 * and refills in flight run across them (they write the ring only).
 * fn = NULL unregisters. */
typedef int (*wpt_exchange_fn)(void* user);
int wpt_set_exchange(wpt_exchange_fn fn, void* user, void* local_dev, void* gathered_dev, uint64_t slot);
/* float4 entries per rank the exchange needs (the largest partition). */
int64_t wpt_exchange_slot(void);

/* Multi-GPU over RCCL (the reference has no collective, its
 * README intends pixel partitions over 8 workers, README.md:87). One process
 * per GPU. Rank 0 makes a 128-byte id with wpt_comm_unique_id and the host
 * hands it to every rank (any channel); every rank then calls wpt_set_comm
 * (collective): its partition = tiles of `tile` px dealt round-robin
 * (wpt_set_partition), plus an RCCL communicator. compute() then traces only
 * the rank's pixels with no communication; with adaptive halves the ranks
 * exchange the frame at round boundaries over the communicator
 * (ncclAllGather), so every rank must pass the same n to compute(). A rank's
 * sample stock (WPT_OPT_STOCK_RANKS) is its own: the collectives do not
 * depend on it.
 * wpt_gather_frame(root) (collective): every rank's partition into the root's
 * frame (grouped ncclSend / ncclRecv over xGMI); results() / read_radiance()
 * on the root then return the whole image. */
int wpt_comm_unique_id(void* out128);
int wpt_set_comm(uint32_t rank, uint32_t nranks, uint32_t tile, const void* unique_id128);
int wpt_gather_frame(uint32_t root);
int wpt_comm_destroy(void);
/* A caller's transport instead of RCCL (another collective library, a host
 * staging path, a test harness). After wpt_set_partition(rank, nranks, tile),
 * register fn with two device buffers of this rank's device: send_dev (slot
 * float4) and recv_dev (nranks * slot float4, rank-major), slot >=
 * wpt_exchange_slot(). The library packs this rank's partition into send_dev
 * (float4 per partition pixel: acc.xyz, count as u32 bits; the device is
 * synchronised) and calls fn(user, op, root):
 *   WPT_XFER_GATHER    (wpt_gather_frame): every rank's send_dev into root's
 *                      recv_dev at slot offset r * slot (gather plan below);
 *   WPT_XFER_ALLGATHER (adaptive round boundaries): the same into every rank's.
 * fn returns 0 once the data is in place (non-zero fails the call); the root
 * then unpacks recv_dev into its frame. Registering a transport replaces
 * (destroys) an RCCL communicator set with wpt_set_comm; a registration the
 * call rejects changes nothing. fn = NULL unregisters the transport only;
 * wpt_set_comm and wpt_comm_destroy drop it. */
#define WPT_XFER_GATHER 0
#define WPT_XFER_ALLGATHER 1
typedef int (*wpt_transport_fn)(void* user, int32_t op, uint32_t root);
int wpt_set_transport(wpt_transport_fn fn, void* user, void* send_dev, void* recv_dev, uint64_t slot);
/* Host-only: the point-to-point transfers of a rooted gather as rank `rank`
 * posts them (what wpt_gather_frame runs over RCCL: grouped ncclSend /
 * ncclRecv): out[4i..4i+3] = {peer, float4 offset in root's buffer, float4
 * count, 1 = receive / 0 = send}; returns the count (nranks - 1 at the root,
 * 1 elsewhere, 0 for one rank). */
int64_t wpt_gather_plan(uint32_t rank, uint32_t nranks, uint32_t root, uint64_t slot, uint64_t* out);
/* Host-only: the sequential f32 sum ((0 + v[0]) + v[1]) + ... bit for bit,
 * as the adaptive rounds compute the reference's mse_sum
 * (sampling_strategy.rs:138-141) — exposed for its tests. */
float wpt_seq_sum(const float* v, uint64_t n);
/* Host-only: the same sum from per-chunk effects (wpt_seqsum.h: the chunks'
 * effects by the host restatement, then the ordered walk the adaptive rounds
 * run) — exposed for its tests. */
float wpt_seq_sum_chunks(const float* v, uint64_t n);
/* The same sum with the chunk effects computed on the session's device
 * (k_sum_chunks / k_sum_scan / k_sum_eff, as every adaptive round does), the
 * walk on the host: *out = the sum. For its tests; needs wpt_init. */
int wpt_seq_sum_device(const float* v, uint64_t n, float* out);
/* Test hook: the error estimate of an adaptive round (sampling_strategy.rs:
 * 122-144) as the session's rounds run it (the same kernels, launch geometry
 * and host walk), on the caller's frame of W x H pixels: acc3 = W*H*3 f32
 * sums, cnt = W*H sample counts. half: 0 the left screen half (x < W/2), 1
 * the right one. mse_out = that half's errors in the half's raster order (its
 * width x H floats; none for an empty half), stats3_out = {sum, min, max} as
 * the planning kernel receives them. Works in buffers of its own: the
 * session's frame, rounds and stock stay as they are. Needs wpt_init;
 * WPT_ERR_INVALID_ARG for a null pointer, half > 1, W*H == 0 or W*H >= 2^32. */
int wpt_adaptive_error(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, uint32_t half, float* mse_out,
                       float* stats3_out);
/* Test hook: the planning part of a round of screen half `half` (:146-172;
 * first != 0: the round after a reset, 4 samples per pixel; adaptive == 0: a
 * random half's round, 1 sample per pixel) from the caller's errors mse_in
 * (the half's raster order), stats3_in = {sum, min, max} and counts cnt_in
 * (W*H): count_out = samples per pixel of the frame (W*H; the other half's
 * are 0), offset_out = their exclusive prefix (W*H + 1; the last entry is the
 * round's length), base_out = the pixels' counts before the round (W*H), samp
 * = the RGBA sampling view (W*H*4), in and out: an estimating round repaints
 * the half, everything else stays as passed in. Same session rules and errors
 * as wpt_adaptive_error. */
int wpt_adaptive_plan(uint32_t W, uint32_t H, uint32_t half, int32_t first, int32_t adaptive, const float* mse_in,
                      const float* stats3_in, const uint32_t* cnt_in, uint32_t* count_out, uint32_t* offset_out,
                      uint32_t* base_out, uint8_t* samp);

/* stats: out[0..39] = paths, rays (primary+extension), shadow rays, BVH node
 * visits, primitive tests, bounce iterations, then per kernel (extend, shadow):
 * node visits, primitive tests, node bytes fetched, then the fast-path rays
 * re-traced by the exact traversal (extend, shadow), then traversal-loop
 * iterations summed over lanes and those with a live ray (extend, shadow),
 * then PNEE photon rays shot and photons stored (tracer.rs:126-152), then
 * the adaptive rounds' error sums: chunks walked, chunks re-summed element
 * by element, and of those the ones copied on demand; then the samples
 * adaptive rounds took from the sample stock (WPT_OPT_STOCK; a sample's
 * rays count when a round takes it) and the paths of a random half traced on
 * the fill lane (WPT_OPT_FILL), then
 * the algorithmic bytes of the fused extend + shadow launches, then the paths
 * RR-only batches handed to k_finish and the most bounces one of them took,
 * then the most node visits of one ray in a fused k_trace launch, then
 * the traversal loop's body SIMD use: lanes about to expand an internal node
 * summed over wave iterations, the iterations in which any lane did, and the
 * same for leaf tests (lanes / bodies <= 64); out[33] = samples traced
 * into the stock (refills and round deficits), out[34] = of those the
 * rounds' deficits, out[35] = rounds that waited for a refill still in
 * flight, out[36..37] = host microseconds in round planning and in the
 * stock's round step, out[38] = rays traced into the stock (extension +
 * shadow; rays and shadow rays count a stocked sample's when a round takes it),
 * out[39] = of rays + shadow rays, those of samples taken from the stock,
 * out[40] = of rays, those their producer resolved (WPT_OPT_PRESOLVE: plane
 * or miss, never fed to a traversal kernel; a stock refill's count when traced),
 * out[41] = of out[40], the rays resolved to a miss that adds nothing to their
 * path and so never written to a ray stream (WPT_OPT_DROP_MISS),
 * out[42] = of shadow rays, those their producer resolved as unoccluded and
 * added itself, never fed to a traversal kernel (WPT_OPT_PRESOLVE_SHADOW),
 * out[43] = of out[40], the primary rays k_generate_shade resolved and shaded
 * itself, never written to a ray stream (WPT_OPT_GEN_SHADE).
 * Visit/test/byte/iteration counts are only gathered with counting on. */
int wpt_stats(uint64_t* out, size_t n);
/* per-kernel device time (profiling on): out[0..11] = {ms, launches} ×
 * {generate, extend, shade, shadow, accumulate, trace (fused extend +
 * shadow)}, summed over launches; the lanes' launches overlap, so
 * out[12..23] = {busy ms, logical launches} per kernel: the union of its
 * launch intervals, and launches counted once per bounce (generate /
 * accumulate: once per batch); out[24..27] = 0 (were the round-4 fast tree's
 * re-trace drains). */
int wpt_kernel_times(double* out, size_t n);
int wpt_set_counting(int on);
int wpt_set_profiling(int on);
/* Concurrent lanes (slices of a batch traced on their own HIP streams) of
 * the next compute calls: 1 .. 8 (default 4). 1 serialises the kernels and
 * gives its traversal kernels the whole GPU (multi-lane batches use
 * WPT_OPT_GRID_PCT of it), so wpt_kernel_times then gives their standalone
 * times. The frame is bit-identical for any count. */
int wpt_set_lanes(int32_t n);
/* Launch configuration (no environment variable changes it; the built-in
 * defaults are the measured production settings). With no
 * session it sets the default of every later wpt_init (WPT_OPT_DEFAULTS
 * restores the built-in ones); with a session it changes that session only
 * (scene / partition rebuilt where the option shapes them, accumulation reset
 * then). The frame is bit-identical for every setting. */
#define WPT_OPT_DEFAULTS 0       /* no session: forget every default set so far (value ignored) */
#define WPT_OPT_TRAVERSAL 1      /* extension rays: 0 exact BVH2, 1 BVH4 fast path + exact re-trace, 3 auto (default: BVH4 on scenes with
                                    other shapes than triangles, else BVH2); 2 (the fast tree) was removed in round 5 */
#define WPT_OPT_TRAVERSAL_SH 2   /* shadow rays: the same choice */
#define WPT_OPT_FUSED 3          /* 1: every batch traces bounce b's extension + b-1's shadow rays in one launch */
#define WPT_OPT_FUSED_BELOW 4    /* batches below this many paths run fused (default 2^24) */
#define WPT_OPT_SMALL_LANES 5    /* lane cap of those small batches (default 2) */
#define WPT_OPT_PIXEL_TILE 6     /* whole sample rounds traced in tiles of this many px (default 8; 0 raster) */
#define WPT_OPT_GRID_PCT 7       /* traversal grids of multi-lane batches, % of resident capacity (default 50) */
#define WPT_OPT_REFILL 8         /* idle lanes of a wave before it takes new extension rays (default 12) */
#define WPT_OPT_REFILL_SH 9      /* the same for shadow rays (default 16) */
#define WPT_OPT_TREELET 10       /* LDS treelet of the BVH2's top node pairs (default 1) */
#define WPT_OPT_BVH_BUILD 11     /* BVH2 build: 0 GPU for >= 65536 finite shapes (default), 1 host, 2 GPU */
#define WPT_OPT_LANES 12         /* as wpt_set_lanes (1..8, default 4; one HIP stream each: more lanes than the process has hardware queues (GPU_MAX_HW_QUEUES, 4 by default) share them) */
#define WPT_OPT_FINISH_BELOW 13  /* RR-only batches: once at most this many paths live, one kernel runs each to its end (default 262144; 0 never) */
#define WPT_OPT_TRACE_GRID_PCT 14 /* grid of the fused k_trace (small batches), % of resident capacity (default 75) */
/* 15-19 and 21 (the fast tree's build and drain options) were removed in round 5 */
#define WPT_OPT_FINISH_EVERY 20  /* RR-only batches: bounces between reads of the live count (a host round trip; default 4) */
#define WPT_OPT_PROBE 22         /* record the wave timelines of the next N traversal launches (wpt_probe_read; default 0 = off) */
#define WPT_OPT_STOCK 23         /* adaptive halves (one rank; several ranks with WPT_OPT_STOCK_RANKS): a ring of this many
                                    samples per pixel of the rank's partition, traced ahead of the rounds by refill batches on
                                    the async lanes; a round adds its samples from it in sample order and traces only what it
                                    lacks (0 off, or a power of two 64..4096; default 1024, halved while partition pixels x
                                    slots exceed 2^32 or the ring 48 GB) */
#define WPT_OPT_STOCK_LANES 24   /* async lanes the refills rotate over, 1..5 (default 2) */
#define WPT_OPT_FILL 25          /* one random + one adaptive half (the reference's init defaults): the random half's whole
                                    rounds outside its 2 seam columns run on the fill lane beside the adaptive half's
                                    rounds (default 0: slower than the main lanes once the stock is on) */
#define WPT_OPT_ASYNC_PRIO 26    /* 1: those async batches on low-priority streams (default 0) */
#define WPT_OPT_ASYNC_GRID_PCT 27 /* their persistent traversal grids, % of the resident capacity (0: the main batches';
                                    default 100) */
#define WPT_OPT_STOCK_AHEAD 30   /* a refill stocks a pixel to c + min(ahead * c + extra, slots - c) samples past its count,
                                    c = its samples in the round just planned (default 40) */
#define WPT_OPT_STOCK_EVERY 32   /* a refill after every this many rounds of a half (default 3) */
#define WPT_OPT_STOCK_EXTRA 33   /* see WPT_OPT_STOCK_AHEAD (default 8) */
#define WPT_OPT_ASYNC_ONESHOT 31 /* 1: async batches' traversal grids cover every ray (one feed chunk per wave), so their blocks
                                    retire with their rays instead of holding CUs for a whole bounce (default 0) */
#define WPT_OPT_STOCK_PREFILL 35 /* 1: each compute call first refills the adaptive halves' stock from their last round's
                                    counts, sized to the call's budget (default 1) */
#define WPT_OPT_ASYNC_FUSED_BELOW 36 /* async batches (stock refills, filler) below this many paths run the fused k_trace
                                      (0: WPT_OPT_FUSED_BELOW; default 2^26) */
#define WPT_OPT_PRESOLVE 37      /* 1 (default): k_generate / k_shade resolve extension rays that provably end on a plane or
                                    in the background (exact root and guard box tests) and keep them out of the traversal
                                    kernels' streams; 0: every ray is traversed. Depth-capped batches on BVH scenes only. */
#define WPT_OPT_DROP_MISS 38     /* 1 (default): a ray its producer resolves to a miss (WPT_OPT_PRESOLVE) whose throughput *
                                    background is +0 in every component, the product the next shade would add, is counted
                                    and written to no stream; 0: it is appended and shaded like any resolved ray */
#define WPT_OPT_PRESOLVE_SHADOW 39 /* 1 (default): k_shade's presolving variants add the NEE contribution of a shadow ray that
                                    provably ends unoccluded (no plane before the light, every guard box missed or behind
                                    it, no other light-guard triangle hit) and write it to no stream; 0: every shadow ray
                                    is traversed. Effective only where WPT_OPT_PRESOLVE is; the frame is the same bits. */
#define WPT_OPT_GEN_SHADE 40     /* 1 (default): batches that presolve, other than PNEE and stock batches, generate their paths
                                    with k_generate_shade: a primary ray it resolves (WPT_OPT_PRESOLVE) is shaded at once, from
                                    registers, instead of being written to the back of stream 0 and read back by k_shade(0);
                                    0: k_generate_ps and k_shade as before. The frame and every count are the same bits. */
#define WPT_OPT_STOCK_RANKS 42   /* 1: sessions with several ranks use the sample stock too: every rank keeps a ring over its own
                                    partition (about 1/N of the one-rank ring) and adds its pixels' share of the global rounds
                                    from it; 0 (default): they trace each round's samples as the round takes them. Changing it
                                    within a session drops the stock as a WPT_OPT_STOCK change does. The frame, the counts, the
                                    sampling view and every ray count are the same bits for both values. */
#define WPT_OPT_STOCK_RING_BYTES 43 /* read-only: bytes of the two ring blocks (radiance + ray counts, refill ids: 20 per slot) of
                                       the session's sample stock as it sized them, 0 while it holds none. A session that stops
                                       using its ring (WPT_OPT_STOCK 0, WPT_OPT_STOCK_RANKS 0, another partition or viewport)
                                       keeps the blocks, and this value, until it sizes its next ring or ends */
#define WPT_OPT_VIEWPORT 44      /* read-only: the session's viewport, width | height << 32 (the size of wpt_first_hit's planes) */
#define WPT_OPT_DENOISE_LDS 45   /* bit i: iteration i of wpt_denoise (step 1 << i, i = 0..2) runs the kernel that stages its tile
                                    and halo in LDS; clear: the kernel that reads its taps from global memory, as steps 8 and
                                    16 always do. The same bits either way (default 7) */
#define WPT_OPT_HISTORY 46       /* read-only: wpt_reproject's history: 0 none, 1 usable, 2 kept in the current accumulation
                                    (wpt_reproject is an error until the next reset) */
#define WPT_OPT_MAP_MODE 47      /* read-only: 1 once wpt_compute_map traced a sample in the current accumulation (wpt_compute is
                                    an error until the next reset), else 0 */
#define WPT_OPT_LOG 34           /* 1: host steps of adaptive rounds / the stock to stderr (debugging; default 0) */
#define WPT_OPT_SCENE_TRAVERSAL 28 /* read-only (wpt_get_option): what the session's scene runs: 0 exact BVH2, 1 BVH4, 2 linear
                                      scan (BVH disabled), -1 no scene */
#define WPT_OPT_OCT_VIEW 41      /* read-only: where the shade kernel reads the session's PNEE octree: 0 global memory, 1 child
                                    array in LDS, 2 child array and CDFs in LDS (-1 no tree yet) */
#define WPT_OPT_SCENE_TRI_ONLY 29 /* read-only: 1 if the scene's finite shapes are all triangles (-1 no scene) */
int wpt_set_option(int32_t option, int64_t value);
/* Wave timelines of the traversal launches recorded since WPT_OPT_PROBE was
 * set (measurement only; the probe costs a clock read per wave and per feed
 * refill, results are the same bits). Returns the launches recorded; with
 * meta and rec non-NULL fills meta[5i..5i+4] = {kernel (1 extend, 3 shadow,
 * 5 fused trace), lane, bounce, waves, first entry} and rec[4e..4e+3] =
 * {start, the moment the wave's work feed ran dry, end, rays taken} per wave
 * entry e (steady-clock ticks, ticks_per_us of them per microsecond), then
 * restarts the recording. With WPT_OPT_PRESOLVE the rays of the bounce that
 * their producer resolved, which no wave takes, are added to the launch's
 * first entry. Call it first with meta = rec = NULL (the size
 * query: it takes the snapshot and sets *rec_entries to the entries rec must
 * hold), then with buffers: *rec_entries = rec's capacity in entries, meta
 * of 5 x the launches the query returned. */
int64_t wpt_probe_read(uint32_t* meta, uint32_t* rec, uint64_t* rec_entries, double* ticks_per_us);
int wpt_get_option(int32_t option, int64_t* value);
/* The active scene's BVH2 build: out[0] = build ms (host wall clock, or the
 * GPU build's device time incl. its copies), out[1] = 1 if it was built on
 * the GPU. Scenes with >= 65536 finite shapes are built on the GPU
 * (wpt_bvh_gpu.h, bvh.rs:103-437 level by level, the same tree);
 * WPT_OPT_BVH_BUILD forces either. */
int wpt_scene_build_info(double* out);
int wpt_clear_stats(void);
int wpt_sync(void);
/* BVH2 depth of the active scene. */
int wpt_bvh_depth(void);

/* Parity hooks: closest hit (Scene::trace_g, scene.rs:162-184) for n rays
 * {ox,oy,oz,dx,dy,dz}; t = +inf and id = -1 on a miss. Shadow query
 * (Scene::shadow_ray, scene.rs:104-133) for {p.xyz, q.xyz} and light shape ids. */
int wpt_trace_rays(size_t n, const float* rays, float* t_out, int32_t* id_out);
int wpt_shadow_rays(size_t n, const float* pq, const int32_t* light, uint8_t* occluded);
/* First-hit feature planes of sample `sample` of every frame pixel (raster order,
 * width*height entries each; any pointer may be NULL = not wanted):
 *  dir3    3 f32  the primary ray's direction (origin = the camera)
 *  t       f32    Scene::trace distance, +inf on a miss      (trace_original_depth, tracer.rs:205-213)
 *  id      i32    shape id in the scene's reordered shape list, -1 on a miss
 *  visits  u32    the reference's num_bvh_hits of this ray   (trace_original_bvh, tracer.rs:216-219)
 *  normal3 3 f32  Hit.normal (faces the ray); +0 on a miss
 *  albedo3 3 f32  Diffuse colour, or the Emissive intensity; +0 on a miss
 *  kind    u8     0 miss, 1 diffuse, 2 emissive
 * The ray is the one wpt_compute traces first for that pixel and sample, and
 * the hit is found by the exact BVH2 on every scene. The whole frame on the
 * calling rank, whatever the partition; the session (accumulation, rounds,
 * sample stock, wpt_stats, wpt_kernel_times) is not touched. With every
 * pointer NULL nothing is launched. WPT_ERR_DEVICE if the traversal stack
 * overflowed (no ray is dropped silently). u8 colour maps of the planes
 * (a depth view, a BVH heat view) are the host's: the reference defines none. */
int wpt_first_hit(uint32_t sample, float* dir3, float* t, int32_t* id, uint32_t* visits,
                  float* normal3, float* albedo3, uint8_t* kind);
/* Host-only (no session, no GPU): the primary rays gen_path makes, 6 f32 per pixel
 * {origin = cam5[0..2], direction}; cam5 = {x, y, z, rot_x, rot_y}. */
int wpt_primary_rays(uint32_t width, uint32_t height, const float* cam5, uint32_t frame_seed,
                     uint32_t sample, float* rays6);
/* Edge-avoiding a-trous filter (Dammertz et al. 2010) of the session's frame as
 * the calling rank holds it, guided by the first-hit planes of sample `sample`
 * (depth, normal, albedo, kind: wpt_first_hit's, made on the device, no host
 * round trip). The stencil is the reference's GAUSS5 (render_target.rs:21-27)
 * at steps 1, 2, 4, ... for `iterations` (1..5) passes; the colour weight
 * 1 / (1 + |dc|^2 / sig^2) starts at sig = sigma_c and halves per pass, the
 * normal weight is max(n_p . n_q, 0)^32, the depth weight 1 / (1 + r^2) with
 * r = |t_p - t_q| / (sigma_z * t_p * step); taps of another kind (miss /
 * diffuse / emissive) or without a finite mean are never read. flags:
 * WPT_DENOISE_ALBEDO filters radiance / albedo on diffuse hits and multiplies
 * the albedo back. The definition to the operation: DESIGN.md §2; every output
 * bit is that of wpt_denoise_host on the same planes while |acc / cnt| <= 2^100.
 *  rgb3   3 f32  the filtered mean; +0 where valid is 0
 *  valid  u8     1 where the pixel has samples and a finite mean (on a partitioned
 *                session the other ranks' pixels have none until wpt_gather_frame)
 *  rgba   4 u8   (clamp(rgb, 0, 1) * 255) as u8, alpha 255 (render_target.rs:62-64)
 * Any output may be NULL; with all of them NULL nothing is launched. The session
 * (accumulation, rounds, sample stock, wpt_stats, wpt_kernel_times) is not touched.
 * WPT_ERR_INVALID_ARG: iterations 0 or above 5, a sigma not finite or <= 0, an
 * unknown flag; for the two functions below also a null input, W*H == 0 or >= 2^32. */
#define WPT_DENOISE_ALBEDO 1u
int wpt_denoise(uint32_t sample, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags, float* rgb3,
                uint8_t* valid, uint8_t* rgba);
/* Test hook: the same kernels and launch geometry on a caller's W x H planes
 * (acc3, cnt as wpt_read_radiance gives them; t, normal3, albedo3, kind as
 * wpt_first_hit does), in buffers of its own. Needs wpt_init. */
int wpt_denoise_planes(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, const float* t,
                       const float* normal3, const float* albedo3, const uint8_t* kind, uint32_t iterations,
                       float sigma_c, float sigma_z, uint32_t flags, float* rgb3, uint8_t* valid, uint8_t* rgba);
/* Host only (no session, no GPU): the filter's restatement, the same functions
 * the kernels call. */
int wpt_denoise_host(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, const float* t,
                     const float* normal3, const float* albedo3, const uint8_t* kind, uint32_t iterations,
                     float sigma_c, float sigma_z, uint32_t flags, float* rgb3, uint8_t* valid, uint8_t* rgba);
/* Reverse reprojection of a kept history frame into the current camera, merged
 * with the session's frame as the calling rank holds it (partitions as in
 * wpt_denoise). The reference resets its accumulation at every camera move
 * (wasm_interface.rs:239-248); its materials are diffuse and emissive only, so
 * what a surface point gathered under the previous camera is valid under the
 * new one. Per pixel, through the first-hit planes of sample `sample` (made on
 * the device): the hit point is projected into the history's view, the four
 * pixels around it (bilinear weights; WPT_REPROJECT_NEAREST: the nearest one)
 * are kept if they have samples and a finite mean, the pixel's kind (with
 * WPT_REPROJECT_SAME_SHAPE also its shape id), a normal with n_p . n_q >=
 * cos_min and a depth within eps_z * (distance to the history's camera); their
 * weighted mean h enters the sums as acc + h * L, cnt + L, where L is the
 * smallest sample count among the kept taps, at most max_len. Misses, pixels
 * with a non-finite sum and pixels without a kept tap pass through unchanged
 * (len 0), as every pixel does while there is no history. The definition to the
 * operation: DESIGN.md §2; every output bit is that of wpt_reproject_host on
 * the same planes while every finite mean and sum is at most 2^100.
 *  acc3  3 f32  the merged sums      cnt  u32  the merged counts
 *  len   u32    L, the history length the pixel received
 * Any output may be NULL; with all of them NULL and no WPT_REPROJECT_KEEP
 * nothing is launched. Without KEEP neither the session (accumulation, rounds,
 * sample stock, wpt_stats, wpt_kernel_times) nor the history changes. With KEEP
 * the merged frame, the planes of `sample` and the camera become the history
 * (nothing else changes). The history outlives whatever only resets the
 * accumulation (camera, settings, render options, partition); a new viewport,
 * a scene upload (wpt_update_scene, a mesh reload, an option that rebuilds the
 * scene), wpt_shutdown and wpt_history_drop drop it. A history kept in the
 * current accumulation already contains its samples: until the next reset
 * wpt_reproject returns WPT_ERR_INVALID_ARG and changes nothing. The intended
 * loop: compute and reproject to display as often as wanted; reproject with
 * KEEP once, right before wpt_update_camera; then compute and reproject again.
 * WPT_ERR_INVALID_ARG: cos_min outside [-1, 1] or eps_z < 0 or either not
 * finite, max_len 0 or above 2^24, an unknown flag (KEEP is one to the two
 * plane functions); for those two also a null input, W*H == 0 or >= 2^32. */
#define WPT_REPROJECT_KEEP 1u        /* session call only */
#define WPT_REPROJECT_NEAREST 2u
#define WPT_REPROJECT_SAME_SHAPE 4u
int wpt_reproject(uint32_t sample, float cos_min, float eps_z, uint32_t max_len, uint32_t flags, float* acc3,
                  uint32_t* cnt, uint32_t* len);
int wpt_history_drop(void);
/* wpt_denoise's filter over the merged frame and the guide planes that the
 * last successful wpt_reproject of this viewport left on the device: preview =
 * reproject + filter without a host round trip. Arguments, outputs and errors
 * as wpt_denoise; every output bit is that of wpt_denoise_host on that call's
 * acc3 / cnt and the first-hit planes of its `sample`. WPT_ERR_INVALID_ARG also
 * if no such call was made since the viewport was set. */
int wpt_denoise_merged(uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags, float* rgb3, uint8_t* valid,
                       uint8_t* rgba);
/* wpt_first_hit's planes for the virtual viewport scale*width x scale*height
 * (raster order, scale^2*width*height entries each) under the session's camera
 * and frame seed: the ray of fine pixel (X, Y) is the one
 * wpt_primary_rays(scale*width, scale*height, cam, seed, sample) gives; the
 * aspect ratio and so the field of view are the session's. scale 1..4; scale 1
 * is wpt_first_hit bit for bit. The planes are made in a buffer of their own:
 * the guides wpt_denoise, wpt_reproject and wpt_sample_map work from are not
 * disturbed, and the session is not touched, as with wpt_first_hit.
 * WPT_ERR_INVALID_ARG: another scale, or scale^2*width*height >= 2^32. */
int wpt_first_hit_scaled(uint32_t scale, uint32_t sample, float* dir3, float* t, int32_t* id, uint32_t* visits,
                         float* normal3, float* albedo3, uint8_t* kind);
/* Guided upsampling of the session's W x H frame to sW x sH (joint bilateral
 * upsampling with albedo demodulation): paths are traced at the session's
 * viewport, the displayed frame takes its geometry (edges, emitters, albedo)
 * from first-hit planes made at the fine viewport, wpt_first_hit_scaled(scale,
 * sample)'s, on the device. The source is the session's frame as the calling
 * rank holds it under the first-hit planes of `sample`, or with
 * WPT_UPSAMPLE_MERGED the merged frame and guide planes the last successful
 * wpt_reproject left on the device (what wpt_denoise_merged reads; the same
 * error when there is none).
 *  Coarse stage: wpt_denoise's pack with WPT_DENOISE_ALBEDO always on (diffuse
 *  pixels hold irradiance = mean / albedo), then `iterations` (0..5; 0: none)
 *  of its passes, WPT_OPT_DENOISE_LDS choosing the kernels as there.
 *  Fine pixel (X, Y) of kind K (the fine planes'):
 *   K = 0  the scene's background, valid 1.   K = 2  the emitter's intensity
 *   (the fine albedo plane), valid 1: exact for every render type, the
 *   reference adds throughput (1,1,1) * intensity at a first hit and returns.
 *   K = 1  a = 2X + 1 - s, x0 = floor(a / 2s), fx = (a - 2s x0) / 2s, likewise
 *   y; the coarse pixels (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with
 *   the bilinear weights of (fx, fy). A tap outside the coarse viewport, not
 *   diffuse, without samples or without a finite value is never read. Weight
 *   w = bilinear * max(N . n_q, 0)^32 * 1 / (1 + r^2), r = |T - t_q| / (sigma_z
 *   * T), with the fine pixel's normal N and depth T; taps with w > 0 are
 *   averaged and the fine pixel's albedo (a component of 0 reads as 1) is
 *   multiplied back: valid 1. If no tap passes, the 4 x 4 coarse block
 *   x0-1..x0+2, y0-1..y0+2 under the same tests with bilinear = 1: valid 2.
 *   If none passes there either: +0, valid 0.
 * The definition to the operation: DESIGN.md §2; every output bit is that of
 * wpt_upsample_host on the same planes while |acc / cnt| <= 2^100. Emitters and
 * misses need no such bound; a coarse pixel without samples or with a
 * non-finite value is never read; nothing crosses a kind edge or a normal edge
 * with dot 0.
 *  rgb3   3 f32  sW x sH     valid  u8  0, 1, 2 as above
 *  rgba   4 u8   (clamp(rgb, 0, 1) * 255) as u8, alpha 255
 * Any output may be NULL; with all of them NULL nothing is launched. The
 * session, the history and the sample map are only read (wpt_stats and
 * wpt_kernel_times too are unchanged).
 * WPT_ERR_INVALID_ARG: scale outside 2..4, iterations above 5, a sigma not
 * finite or <= 0, an unknown flag (MERGED is one to the two functions below),
 * scale^2*W*H >= 2^32; for the two functions below also a null input or W*H == 0. */
#define WPT_UPSAMPLE_MERGED 1u       /* session call only */
int wpt_upsample(uint32_t scale, uint32_t sample, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags,
                 float* rgb3, uint8_t* valid, uint8_t* rgba);
/* Test hook: the same kernels and launch geometry on a caller's planes, in
 * buffers of its own: the coarse W x H frame and guides (as wpt_denoise_planes
 * takes them), the fine sW x sH guides (as wpt_first_hit_scaled gives them)
 * and the background's 3 f32. Needs wpt_init. */
int wpt_upsample_planes(uint32_t W, uint32_t H, uint32_t scale, const float* acc3, const uint32_t* cnt, const float* t,
                        const float* normal3, const float* albedo3, const uint8_t* kind, const float* hi_t,
                        const float* hi_normal3, const float* hi_albedo3, const uint8_t* hi_kind,
                        const float* background3, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags,
                        float* rgb3, uint8_t* valid, uint8_t* rgba);
/* Host only (no session, no GPU): the restatement, the same functions the
 * kernels call. */
int wpt_upsample_host(uint32_t W, uint32_t H, uint32_t scale, const float* acc3, const uint32_t* cnt, const float* t,
                      const float* normal3, const float* albedo3, const uint8_t* kind, const float* hi_t,
                      const float* hi_normal3, const float* hi_albedo3, const uint8_t* hi_kind,
                      const float* background3, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags,
                      float* rgb3, uint8_t* valid, uint8_t* rgba);
/* Test hook: the same kernel and launch geometry on a caller's W x H planes, in
 * buffers of its own, no state kept. cam3: the current camera's position; acc3,
 * cnt as wpt_read_radiance gives them; dir3, t, id, normal3, kind as
 * wpt_first_hit does; prev_cam5 = {x, y, z, rot_x, rot_y} and the h_ planes:
 * the history. Needs wpt_init. */
int wpt_reproject_planes(uint32_t W, uint32_t H, const float* cam3, const float* acc3, const uint32_t* cnt,
                         const float* dir3, const float* t, const int32_t* id, const float* normal3,
                         const uint8_t* kind, const float* prev_cam5, const float* h_acc3, const uint32_t* h_cnt,
                         const float* h_t, const int32_t* h_id, const float* h_normal3, const uint8_t* h_kind,
                         float cos_min, float eps_z, uint32_t max_len, uint32_t flags, float* acc3_out,
                         uint32_t* cnt_out, uint32_t* len_out);
/* Host only (no session, no GPU): the restatement, the same functions the
 * kernel calls. */
int wpt_reproject_host(uint32_t W, uint32_t H, const float* cam3, const float* acc3, const uint32_t* cnt,
                       const float* dir3, const float* t, const int32_t* id, const float* normal3, const uint8_t* kind,
                       const float* prev_cam5, const float* h_acc3, const uint32_t* h_cnt, const float* h_t,
                       const int32_t* h_id, const float* h_normal3, const uint8_t* h_kind, float cos_min, float eps_z,
                       uint32_t max_len, uint32_t flags, float* acc3_out, uint32_t* cnt_out, uint32_t* len_out);
/* Guided sampling, the planning half: a sample map (width*height u32, raster
 * order) from the session's counts cnt, the history length len that the last
 * successful wpt_reproject since the last reset of the accumulation gave each
 * pixel (0 everywhere if there was none) and the partition. Per pixel, with
 * e = min(cnt + len, 2^32 - 1):
 *   need = 0 outside the calling rank's partition;
 *   with WPT_MAP_MISS_ONCE, where sample `sample`'s primary ray misses (the
 *     first-hit kind, made on the device): 1 if cnt == 0, else 0 (a caller's
 *     approximation, off by default: `sample` is read under this flag only);
 *   otherwise min(target > e ? target - e : 0, max_per_pixel).
 * T = the sum of the needs. With budget == 0 or T <= budget, count = need.
 * Otherwise the budget is dealt in proportion, exactly: with P the exclusive
 * prefix of the needs in raster order, count[p] = floor(P[p+1] * budget / T) -
 * floor(P[p] * budget / T) in u64. Then the counts sum to budget, count <= need,
 * and count == 0 where need == 0. All of it is integer arithmetic: every output
 * bit is that of wpt_sample_map_host on the same planes.
 *  count_out  width*height u32 (may be NULL)
 *  total_out  2 u64: {T, the sum of the counts} (may be NULL)
 * The map stays on the device for wpt_compute_map until the accumulation is
 * reset (camera, settings, render options, partition, viewport, scene). The
 * session (accumulation, rounds, sample stock, wpt_stats, wpt_kernel_times,
 * history) is not touched. WPT_ERR_INVALID_ARG: target 0, max_per_pixel 0, an
 * unknown flag, T >= 2^32 (lower max_per_pixel; no map is kept); for the two
 * functions below also a null input, W*H == 0 or >= 2^32 - 1. The definition to
 * the operation: DESIGN.md §2. */
#define WPT_MAP_MISS_ONCE 1u
int wpt_sample_map(uint32_t sample, uint32_t target, uint32_t max_per_pixel, uint32_t budget, uint32_t flags,
                   uint32_t* count_out, uint64_t* total_out);
/* Test hook: the same kernels and launch geometry on a caller's W x H planes
 * (cnt as wpt_read_radiance gives it, len as wpt_reproject does, kind as
 * wpt_first_hit does, member: u8, 1 for the pixels of the partition), in buffers
 * of its own, no state kept. Needs wpt_init. */
int wpt_sample_map_planes(uint32_t W, uint32_t H, const uint32_t* cnt, const uint32_t* len, const uint8_t* kind,
                          const uint8_t* member, uint32_t target, uint32_t max_per_pixel, uint32_t budget,
                          uint32_t flags, uint32_t* count_out, uint64_t* total_out);
/* Host only (no session, no GPU): the restatement, the same functions the
 * kernels call. */
int wpt_sample_map_host(uint32_t W, uint32_t H, const uint32_t* cnt, const uint32_t* len, const uint8_t* kind,
                        const uint8_t* member, uint32_t target, uint32_t max_per_pixel, uint32_t budget, uint32_t flags,
                        uint32_t* count_out, uint64_t* total_out);
/* Guided sampling, the tracing half: traces a sample map. count: width*height
 * u32 in raster order, or NULL for the map the last successful wpt_sample_map
 * of the current accumulation left on the device (none: WPT_ERR_INVALID_ARG).
 * Every pixel p of the calling rank's partition, in partition order, gets the
 * samples s = cnt[p] .. cnt[p] + count[p] - 1 (cnt as wpt_read_radiance gives
 * it): paths path_seed(frame_seed, p, s) with the render type of p's screen
 * half, the session's depth cap and light-debug setting, added to the pixel's
 * sum in sample order after what it holds; its count grows by count[p]. Entries
 * of other ranks' pixels are ignored; several ranks need no collective. This is
 * exact at any moment of a session, because every producer of samples leaves a
 * pixel holding exactly the samples 0 .. cnt - 1. The call first waits for the
 * sample stock's refills in flight, as wpt_sync does; the stock is not read
 * again. The frame is the same bits for every batch size, lane count and launch
 * option; wpt_stats and wpt_kernel_times count the paths and rays as any
 * batch's; PNEE halves build or reuse the session's octree as wpt_compute does.
 * Map mode: a call that traced at least one sample puts the session into map
 * mode (WPT_OPT_MAP_MODE reads 1). The random and adaptive sequences take their
 * sample indices from round and position counters, not from the counts, so
 * until the next reset of the accumulation wpt_compute returns
 * WPT_ERR_INVALID_ARG and changes nothing; further maps may be traced. A map of
 * zeros succeeds, launches nothing and does not enter map mode.
 * WPT_ERR_INVALID_ARG, with nothing traced: the partition's counts sum to more
 * than 2^32 - 1, or a pixel's cnt + count exceeds 2^32 - 1. */
int wpt_compute_map(const uint32_t* count);
/* Radiance along a caller's rays: a ray query is a camera path whose primary
 * ray the caller supplies (light probes, irradiance at surface points, panorama,
 * fisheye, orthographic or stereo cameras, a host that builds its own primary
 * rays). Ray i = {ox,oy,oz,dx,dy,dz} as wpt_trace_rays takes them; its key k_i =
 * keys[i], or i if keys is NULL; its samples are s = sample .. sample + spp - 1.
 * The path of (i, s) has the xorshift32 stream path_seed(frame_seed, k_i, s)
 * advanced by two draws (the two jitter draws of a camera ray, taken and
 * discarded), throughput (1,1,1), origin and direction as given, and then
 * trace_original_color's loop (src/tracer.rs) exactly as the session's
 * batches run it for a camera path of render type `type` (WPT_NO_NEE,
 * WPT_NORMAL_NEE, WPT_PNEE), under the session's scene, depth cap, frame seed
 * and light-debug setting; WPT_PNEE builds or reuses the session's octree as
 * wpt_compute does. The direction is used as given, not re-normalised: unit
 * length is the caller's contract, and wpt_primary_rays' directions pass through
 * bit for bit, so with rays6 = wpt_primary_rays(W, H, cam, seed, s), keys NULL
 * and spp 1 the result is sample s of every pixel of a W x H frame of that
 * render type, and the ray counts are that frame's.
 *  rgb3    3 f32  ((+0 + c_0) + c_1) + ... over the ray's samples in sample
 *                 order (RenderTarget::write's sum); the mean is the caller's
 *                 division
 *  status  u8     1 traced; 0 for a ray with a non-finite component or a
 *                 direction of three zeros: not traced, rgb3 +0, no path and no
 *                 ray counted. May be NULL.
 * Ray i's result depends on (ray, key, sample, spp, type), the scene and the
 * render options only: not on n, its position, the other rays, the batch size,
 * the lane count, the partition (any rank answers any ray, no collective) or any
 * wpt_set_option setting. The session is not touched: accumulation, counts,
 * rounds and their positions, sample stock, sampling view, history, sample map
 * and map mode stay as they are, and a wpt_compute after a query continues as if
 * the query had not happened. The call first waits for the sample stock's
 * refills in flight, as wpt_sync does; wpt_stats and wpt_kernel_times count its
 * paths and rays as any batch's. flags: WPT_RAYS_DEVICE: rays6, keys, rgb3 and
 * status are device pointers on the session's device (the call still returns
 * synchronised). Inputs and outputs must not overlap. n == 0 succeeds, launches
 * nothing and waits for nothing.
 * WPT_ERR_INVALID_ARG, with nothing launched and nothing written: n > 0 with a
 * null rays6 or rgb3, spp 0, type > 2, an unknown flag, sample + spp - 1 >
 * 2^32 - 1, n >= 2^32. The definition to the operation: DESIGN.md §2. */
#define WPT_RAYS_DEVICE 1u
int wpt_radiance_rays(size_t n, const float* rays6, const uint32_t* keys, uint32_t sample, uint32_t spp,
                      uint32_t type, uint32_t flags, float* rgb3, uint8_t* status);
/* Host only (no session, no GPU): the status rule above on n rays. */
int wpt_rays_valid(size_t n, const float* rays6, uint8_t* status);
/* Hemisphere gathers at a caller's points (lightmap texels, probe grids, vertex
 * irradiance): a point query is a ray query whose ray the device makes, a new
 * direction for every sample. Record i = {px,py,pz, nx,ny,nz} (24 bytes, the
 * layout of a ray); the normal is used as given, unit length is the caller's
 * contract. Key k_i = keys[i], or i if keys is NULL; samples s = sample ..
 * sample + spp - 1. For (i, s), with the project's f32 operations (wpt_math.h):
 *   st  = path_seed(frame_seed, k_i, s)
 *   r1  = xs_next(st); r2 = xs_next(st)      the two jitter draws of a camera path
 *   ang = (2 * pi) * r1
 *   WPT_POINTS_COSINE: x = cos(ang) * sqrt(1 - r2), y = sqrt(r2), z = sin(ang) * sqrt(1 - r2)
 *                      (sample_hemisphere, src/material.rs)
 *   WPT_POINTS_SPHERE: y = 1 - 2 * r2, q = sqrt(1 - y * y), x = cos(ang) * q, z = sin(ang) * q
 *                      (uniform over the sphere, the normal its pole: probes in free space)
 *   xn  = orthogonal(n), zn = cross(n, xn)
 *   wi  = normalize((xn * x + n * y) + zn * z)
 *   o   = p + wi * 0.0002                    as a bounce leaves a hit point
 * and the path is wpt_radiance_rays' path of the ray (o, wi) on the stream st as
 * it stands (a query path's state after its two discarded draws): throughput
 * (1,1,1), render type `type`, the session's scene, depth cap, frame seed and
 * light-debug setting. So always
 *   rgb3[i] == ((+0 + c_0) + c_1) + ...      (f32, sample order)
 *   c_j = wpt_radiance_rays(1, wpt_point_rays(record i, k_i, sample + j), &k_i, sample + j, 1, type)
 * The caller's estimators: irradiance = pi * rgb3 / spp for WPT_POINTS_COSINE,
 * mean radiance = rgb3 / spp for WPT_POINTS_SPHERE.
 *  status  u8     wpt_rays_valid's rule on the record's six floats: 1, or 0 for a
 *                 non-finite component or a normal of three zeros (not traced,
 *                 rgb3 +0, no path and no ray counted). May be NULL.
 * A sample whose generated ray (o, wi) fails that rule (only normals far from
 * unit length give one) is not traced either: it adds +0 and counts no path and
 * no ray, as the ray query treats that ray; the record's status stays 1.
 * Everything else is wpt_radiance_rays': a result depends on (record, key,
 * sample, spp, type, dist), the scene and the render options only; the session
 * is not touched; the call waits for stock refills as wpt_sync does; wpt_stats
 * and wpt_kernel_times count its paths and rays as any batch's; flags:
 * WPT_RAYS_DEVICE: points6, keys, rgb3 and status are device pointers; n == 0
 * succeeds and launches nothing.
 * WPT_ERR_INVALID_ARG, with nothing launched and nothing written: n > 0 with a
 * null points6 or rgb3, spp 0, type > 2, dist > 1, an unknown flag, sample +
 * spp - 1 > 2^32 - 1, n >= 2^32. The definition to the operation: DESIGN.md §2. */
#define WPT_POINTS_COSINE 0
#define WPT_POINTS_SPHERE 1
int wpt_radiance_points(size_t n, const float* points6, const uint32_t* keys, uint32_t sample, uint32_t spp,
                        uint32_t type, uint32_t dist, uint32_t flags, float* rgb3, uint8_t* status);
/* Host only (no session, no GPU): the ray (o, wi) of every record for ONE sample
 * index, the same code the kernels run; an invalid record gives six +0. A
 * generated ray that is itself invalid is given as computed. */
int wpt_point_rays(size_t n, const float* points6, const uint32_t* keys, uint32_t frame_seed, uint32_t sample,
                   uint32_t dist, float* rays6);
/* Spherical-harmonic projection of a point's gathers (probe grids): the samples
 * of wpt_radiance_points, each weighted by the real SH basis of its own
 * direction. Records, keys, samples, type, dist, status and flags are
 * wpt_radiance_points'. nc = (order + 1)^2 coefficients, order 0 .. 2. With
 *   (o_j, w_j) = wpt_point_rays(record i, k_i, sample + j)
 *   c_j        = wpt_radiance_rays(1, (o_j, w_j), &k_i, sample + j, 1, type)
 * always
 *   sh[(i * nc + k) * 3 + ch] == ((+0 + Y_k(w_0) * c_0.ch) + Y_k(w_1) * c_1.ch) + ...
 * in f32, in sample order, one rounding per product and per addition. The
 * basis (wpt_sh_basis): world axes, z the polar axis, no Condon-Shortley sign,
 * the direction (x, y, z) used as given, each operation one f32 rounding:
 *   Y0 = C0
 *   Y1 = C1 * y          Y2 = C1 * z          Y3 = C1 * x
 *   Y4 = C2 * (x * y)    Y5 = C2 * (y * z)    Y7 = C2 * (x * z)
 *   Y6 = C3 * ((3 * (z * z)) - 1)
 *   Y8 = C4 * ((x * x) - (y * y))
 * C0 .. C4 the f32 nearest to sqrt(1 / 4pi), sqrt(3 / 4pi), sqrt(15 / 4pi),
 * sqrt(5 / 16pi), sqrt(15 / 16pi). The coefficients of a lower order are the
 * leading coefficients of a higher order, bit for bit.
 * A sample that is not traced (an invalid record, or an invalid generated ray)
 * adds nothing to any coefficient; an invalid record's row is all +0.
 * The caller's estimators: for WPT_POINTS_SPHERE, 4 pi / spp * sh estimates the
 * SH coefficients of the incoming radiance; for WPT_POINTS_COSINE, pi / spp * sh
 * those of the radiance times the cosine about the normal.
 * Everything else is wpt_radiance_points': a result depends on (record, key,
 * sample, spp, type, dist, order), the scene and the render options only (not on
 * WPT_SH_CHUNK, the records one internal pass takes); the session is not touched;
 * stock refills, wpt_stats, wpt_kernel_times, WPT_RAYS_DEVICE and n == 0 as there.
 * WPT_ERR_INVALID_ARG, with nothing launched and nothing written: that call's
 * cases with sh in place of rgb3, and order > WPT_SH_MAX_ORDER. The definition
 * to the operation: DESIGN.md §2. */
#define WPT_SH_MAX_ORDER 2
#define WPT_SH_CHUNK 262144
int wpt_probe_sh(size_t n, const float* points6, const uint32_t* keys, uint32_t sample, uint32_t spp,
                 uint32_t type, uint32_t dist, uint32_t order, uint32_t flags, float* sh, uint8_t* status);
/* Host only (no session, no GPU): the (order + 1)^2 basis values of each of n
 * directions {x, y, z}, the same code the kernel runs. WPT_ERR_INVALID_ARG for
 * a null pointer with n > 0 or order > WPT_SH_MAX_ORDER. */
int wpt_sh_basis(size_t n, const float* dirs3, uint32_t order, float* out);
/* First-hit feature planes along a caller's rays: wpt_first_hit's planes for
 * rays that are not the session camera's (the guide planes of a fisheye,
 * panorama, orthographic or stereo frame traced through wpt_radiance_rays).
 * Ray i = {ox,oy,oz,dx,dy,dz} as wpt_radiance_rays takes it, the direction used
 * as given; entry i of every plane is what wpt_first_hit gives a pixel whose
 * primary ray is ray i (n entries each; any pointer may be NULL = neither
 * computed nor stored):
 *  t       f32    Scene::trace distance, +inf on a miss
 *  id      i32    shape id in the scene's reordered shape list, -1 on a miss
 *  visits  u32    the reference's num_bvh_hits of this ray
 *  normal3 3 f32  Hit.normal (faces the ray); +0 on a miss
 *  albedo3 3 f32  Diffuse colour, or the Emissive intensity; +0 on a miss
 *  kind    u8     0 miss, 1 diffuse, 2 emissive
 *  status  u8     wpt_rays_valid's rule: 1 traced, 0 not
 * The hit is found by the exact BVH2 on every scene. A ray of status 0 is never
 * started: t +inf, id -1, visits 0, normal and albedo +0, kind 0. With
 * rays6 = wpt_primary_rays(W, H, cam, seed, s) the planes are wpt_first_hit(s)
 * of a W x H session under that camera and seed, visits included. Ray i's
 * entries depend on that ray and the scene only. The call needs a session and
 * a scene, no viewport, and works in a buffer of its own: the session
 * (accumulation, rounds, sample stock, history, sample map and map mode,
 * wpt_stats, wpt_kernel_times) and the guide planes wpt_denoise, wpt_reproject,
 * wpt_upsample and wpt_sample_map keep on the device are not touched. flags:
 * WPT_RAYS_DEVICE: every pointer is a device pointer on the session's device
 * (the call still returns synchronised). With every output NULL, or n == 0,
 * nothing is launched and the call succeeds.
 * WPT_ERR_INVALID_ARG, with nothing launched and nothing written: n > 0 with an
 * output wanted and a null rays6, an unknown flag, n >= 2^32. WPT_ERR_DEVICE if
 * the traversal stack overflowed, as for wpt_first_hit. */
int wpt_first_hit_rays(size_t n, const float* rays6, uint32_t flags, float* t, int32_t* id, uint32_t* visits,
                       float* normal3, float* albedo3, uint8_t* kind, uint8_t* status);
/* A filtered frame along a W x H grid of a caller's rays: ray y * W + x is pixel
 * (x, y). A composition of three public calls, kept on the device:
 *  raw3, status       what wpt_radiance_rays(W * H, rays6, keys, sample, spp, type,
 *                     ...) gives; wpt_stats and wpt_kernel_times grow, and the
 *                     session is left, exactly as by that call
 *  rgb3, valid, rgba  wpt_denoise_host(W, H, acc3 = raw3, cnt, t, normal3, albedo3,
 *                     kind, iterations, sigma_c, sigma_z, dn_flags) with
 *                     cnt[i] = spp * status[i] and the guide planes
 *                     wpt_first_hit_rays gives for the same rays, bit for bit
 *                     while |acc / cnt| <= 2^100 (wpt_denoise's bound)
 * The sums, the counts, the guide planes and the filter's scratch stay on the
 * device from the first launch to the last; only the outputs asked for are
 * copied. A grid of more rays than the query traces at a time is still filtered
 * as one frame. WPT_OPT_DENOISE_LDS chooses the kernels as for wpt_denoise.
 * flags: WPT_RAYS_DEVICE: every pointer is a device pointer. Any output may be
 * NULL; with all five NULL nothing is launched. Accumulating over several calls
 * is the caller's, as with wpt_radiance_rays.
 * WPT_ERR_INVALID_ARG, with nothing launched and nothing written: W * H == 0 or
 * >= 2^32, a null rays6, spp 0, type > 2, sample + spp - 1 > 2^32 - 1,
 * iterations 0 or above 5, a sigma not finite or <= 0, an unknown bit in flags
 * or dn_flags. The definition to the operation: DESIGN.md §2. */
int wpt_denoise_rays(uint32_t W, uint32_t H, const float* rays6, const uint32_t* keys, uint32_t sample,
                     uint32_t spp, uint32_t type, uint32_t iterations, float sigma_c, float sigma_z,
                     uint32_t dn_flags, uint32_t flags, float* rgb3, uint8_t* valid, uint8_t* rgba,
                     float* raw3, uint8_t* status);
/* Test hook: the producers' presolve of extension rays (WPT_OPT_PRESOLVE) on
 * the device for n rays {ox,oy,oz,dx,dy,dz}: resolved[i] = 1 if ray i needs no
 * traversal; (t, id) is then its closest hit (a plane, or +inf and -1). */
int wpt_presolve_rays(size_t n, const float* rays, uint8_t* resolved, float* t_out, int32_t* id_out);
/* Test hook: k_shade's presolve of shadow rays (WPT_OPT_PRESOLVE_SHADOW) on
 * the device for n pairs {p.xyz, q.xyz} and light shape ids, the ray formed
 * as by wpt_shadow_rays: resolved[i] = 1 if ray i provably ends unoccluded. */
int wpt_presolve_shadow_rays(size_t n, const float* pq, const int32_t* light, uint8_t* resolved);

/* Tear the session down (the reference never does); allows a new wpt_init.
 * The sample stock's two ring blocks (about 42 GB at 1080p) stay with the
 * process for the next session's ring on the device (at most 4 blocks);
 * they are freed when an allocation would otherwise fail. */
int wpt_shutdown(void);

/* Host-only scene inspection (no GPU): builds a scene like wpt_init would and
 * exposes the reordered shapes and the BVH2 nodes for structural parity. */
void* wpt_debug_scene_new(int32_t scene_id, const float* mesh_vertices, size_t num_vertices);
/* out[0..7] = shapes, infinite shapes, nodes, lights, BVH depth, use_bvh, tri_only, BVH4 nodes */
int wpt_debug_scene_info(void* h, uint64_t* out);
/* The BVH4 (bvh4.rs:37-281 DP tree cut, F4 leaf fix): 37 u32 per node =
 * num_children, then per child slot {kind (0 empty, 1 node, 2 leaf), node
 * index | first shape, leaf count, 6 f32 bounds bits}. */
int wpt_debug_scene_nodes4(void* h, uint32_t* out);
/* 8 u32 per node: 6 f32 bounds bits (x_min,y_min,z_min,x_max,y_max,z_max), left_first, count */
int wpt_debug_scene_nodes(void* h, uint32_t* out);
/* 16 f32 per shape: geometry[12] as in wpt_scene.h, kind, emissive, 0, 0 */
int wpt_debug_scene_shapes(void* h, float* out);
/* 4 f32 per shape: the Diffuse colour or the Emissive intensity (rgb), 1 if emissive
 * (the rows of wpt_debug_scene_shapes stay geometry only) */
int wpt_debug_scene_materials(void* h, float* out);
int wpt_debug_scene_lights(void* h, uint32_t* out);
/* The presolve's host restatement over the scene (as wpt_presolve_rays). */
int wpt_debug_scene_presolve(void* h, size_t n, const float* rays, uint8_t* resolved, float* t_out, int32_t* id_out);
/* Its guard boxes: *num_guards (0..4); boxes (may be NULL) = 30 f32: the BVH2
 * root's bounds, then 4 guards (x_min,y_min,z_min,x_max,y_max,z_max);
 * leaf_guard (may be NULL) = per BVH2 node the guard of a leaf, ~0 otherwise. */
int wpt_debug_scene_guards(void* h, uint32_t* num_guards, float* boxes, uint32_t* leaf_guard);
/* The shadow presolve's host restatement (as wpt_presolve_shadow_rays). */
int wpt_debug_scene_presolve_shadow(void* h, size_t n, const float* pq, const int32_t* light, uint8_t* resolved);
/* Its light guards: *light_guards = bit g set if guard g holds emissive
 * triangles only; *num = their primitives together (0..4); ids (may be NULL)
 * = 4 shape ids, -1 beyond *num. */
int wpt_debug_scene_guard_lights(void* h, uint32_t* light_guards, uint32_t* num, int32_t* ids);
void wpt_debug_scene_free(void* h);
/* The same scene with its BVH2 built on the GPU (the device of
 * wpt_set_device, default 0) whatever its size; same accessors. */
void* wpt_debug_scene_new_gpu(int32_t scene_id, const float* mesh_vertices, size_t num_vertices);
/* out[0] = BVH2 build ms, out[1] = 1 if built on the GPU. */
int wpt_debug_scene_build_info(void* h, double* out);

#ifdef __cplusplus
}
#endif

#endif /* WPT_H */
