// wpt_render.h — the wavefront renderer behind the C ABI.
//
// One Renderer per process/GPU. It owns the device copy of the scene, the
// accumulation buffers of its pixel partition and the per-path SoA state of
// the wavefront pipeline (generate → [extend → shade → shadow]* → accumulate),
// replacing RenderInstance::compute_rays + trace_original_color
// (src/tracer.rs:156-330) for a whole batch of paths at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <algorithm>
#include <deque>
#include <vector>

#include "wpt_devmem.h"
#include "wpt_photon.h"
#include "wpt_post.h"
#include "wpt_scene.h"
#include "wpt_seqsum.h"

namespace wpt {

constexpr int kMaxInf = 16;       // infinite shapes (planes) kept in the kernel argument block
constexpr int kMaxBvhDepth = 4096;  // traversal stack: LDS slots + global spill sized from the BVH depth
constexpr int kMaxBounces = 512;  // hard cap for the RR-only (unbounded) mode

// Read-only scene view passed by value to the kernels.
struct DevScene {
  const float4* nodes;      // BVH2: 2 float4 per node (bounds, left_first, count)
  const float4* tree;       // LDS treelet source: 4 float4 per node pair (wpt_render.hip kTreePairs)
  uint32_t tree_pairs, tree_root_lf;
  const float4* prims;      // 4 float4 per finite shape (shape index - num_inf)
  const uint32_t* kinds;    // ShapeKind per finite shape
  const float4* all;        // 4 float4 per shape, every shape (linear scan, BVH disabled)
  const uint32_t* all_kinds;
  const float4* mats;       // per shape: rgb (colour or intensity), w = 1 if emissive
  const float4* lights;     // 5 float4 per light: (v0,area) (v1,shape id) (v2,-) (n,-) (I,-)
  const float4* nodes4;     // fast-path BVH4: 8 float4 (128 B) per node (wpt_scene.h Node4)
  const uint32_t* leaf_table;
  uint32_t num_inf, num_finite, num_shapes, num_lights;
  uint32_t use_bvh, tri_only;
  uint32_t refill_lanes;     // persistent kernels refill idle lanes once this many are idle
  uint32_t refill_lanes_sh;  // (the same for the shadow kernel)
  int stack_cap;             // traversal stack entries per lane (LDS slots + spill)
  uint32_t* overflow;        // device flag: a traversal stack would have overflowed
  const uint32_t* oct_child;  // PNEE octree (wpt_photon.h): first child per node, 0 = leaf
  const float* oct_cum;       // frozen cum_bins, num_lights per node
  const uint32_t* oct_corners;  // per node x 8 offset cases: the 8 cells of the trilinear mix (null: walk them)
  uint32_t oct_nodes;         // 0: no tree (PNEE paths then cannot run)
  uint32_t oct_lds_words;     // words of the tree k_shade copies to LDS: nodes (child) [+ nodes * lights (cum)], 0 = none
  float bg[3];
  float4 planes[kMaxInf];   // infinite shapes: (normal.xyz, normal·location)
  // wave timeline probe (WPT_OPT_PROBE) of this launch, or null: per wave of
  // the grid {start, feed ran dry, end (steady clock ticks), rays taken}
  uint4* probe;
  // presolve (wpt_presolve.h): root and guard boxes; num_guards 0 = resolves
  // nothing. In device memory, not in the argument block: k_shade then loads
  // them where it uses them, not ahead of its loop (30 SGPRs held across
  // shade_path spilled into VGPRs: 75-77 instead of 72). The last member:
  // the kernels that do not read it keep their argument offsets.
  const PresolveBoxes* pre;
};

struct Stats {
  uint64_t paths = 0;
  uint64_t rays = 0;          // primary + extension (extend launches)
  uint64_t shadow_rays = 0;
  uint64_t node_visits = 0;   // only when counting is enabled
  uint64_t prim_tests = 0;
  uint64_t bounces = 0;       // bounce iterations executed
  // per-kernel work split (counting on): extend / shadow
  uint64_t ext_visits = 0, ext_tests = 0, ext_node_bytes = 0;
  uint64_t sh_visits = 0, sh_tests = 0, sh_node_bytes = 0;
  uint64_t fallback_ext = 0, fallback_sh = 0;  // fast-path rays re-traced exactly (tie / quirk)
  // traversal-loop bodies (counting on): lanes that expand an internal node /
  // test a leaf per wave iteration, and the iterations in which each body ran
  uint64_t ex_body_lanes = 0, ex_bodies = 0, lf_body_lanes = 0, lf_bodies = 0;
  // traversal loop iterations summed over lanes, and those with a live ray
  // (counting on): live/lane = SIMD occupancy of the traversal loop
  uint64_t ext_lane_iters = 0, ext_live_iters = 0, sh_lane_iters = 0, sh_live_iters = 0;
  // PNEE preprocessing (tracer.rs:126-152): photon rays shot, photons stored
  uint64_t photon_rays = 0, photons = 0;
  // algorithmic bytes of the fused extend + shadow launches (counting on),
  // with bench.py's per-ray formula
  uint64_t trace_bytes = 0;
  uint64_t max_ray_visits = 0;  // the most node visits of one ray in a fused k_trace (counting on)
  // adaptive rounds' error sums: chunks walked, re-summed element by element,
  // and of those copied on demand (not packed by k_sum_pack)
  uint64_t sum_chunks = 0, sum_resummed = 0, sum_fetched = 0;
  // RR-only tails run by k_finish: paths handed over, and the most bounces
  // one of them still took (the tail's length)
  uint64_t finish_paths = 0, finish_max_bounces = 0;
  // adaptive halves' sample stock (wpt_stock.h): samples traced into it
  // (refills and round deficits) and samples the rounds took from it; a
  // random half's paths traced on the fill lane
  uint64_t stock_traced = 0, stock_consumed = 0, fill_paths = 0;
  // of those: traced by the rounds themselves (their deficits), and rounds
  // whose samples were not all traced when the round wanted them; host time
  // (us) in round planning and in the stock's round step
  uint64_t stock_deficit = 0, stock_waits = 0, plan_us = 0, stock_us = 0;
  uint64_t stock_rays = 0;  // rays traced into the stock (they count in rays / shadow_rays when consumed)
  uint64_t stock_rays_used = 0;  // of rays + shadow_rays: those of samples taken from the stock
  uint64_t presolved_rays = 0;   // of rays: resolved by their producer (wpt_presolve.h), never fed to k_extend / k_trace
  uint64_t dropped_rays = 0;     // of presolved_rays: resolved to a miss that adds nothing, never written to a stream (WPT_OPT_DROP_MISS)
  uint64_t shadow_presolved_rays = 0;  // of shadow_rays: resolved unoccluded by k_shade, never fed to k_shadow / k_trace (WPT_OPT_PRESOLVE_SHADOW)
  uint64_t gen_shaded_rays = 0;  // of presolved_rays: primary rays shaded by k_generate_shade, never written to a stream (WPT_OPT_GEN_SHADE)
};

// Kernel-time accumulators (ms), filled when profiling is on.
// The lanes' launches of one kernel overlap in time: busy[k] = the union of
// kernel k's launch intervals (time during which at least one of its launches
// was in flight), logical[k] = launches counted once per batch step (generate /
// accumulate: one per batch; extend / shade / shadow: one per bounce).
// trace = the fused extend + shadow kernel (k_trace).
// retrace: unused since round 5 (the fast tree's drains; kept so that
// wpt_kernel_times keeps its layout, always 0).
constexpr int kTimedKernels = 7;
struct KernelTimes {
  double generate = 0, extend = 0, shade = 0, shadow = 0, accumulate = 0, trace = 0, retrace = 0;
  uint64_t n_extend = 0, n_shadow = 0, n_shade = 0, n_generate = 0, n_accumulate = 0, n_trace = 0, n_retrace = 0;
  double busy[kTimedKernels] = {0, 0, 0, 0, 0, 0, 0};
  uint64_t logical[kTimedKernels] = {0, 0, 0, 0, 0, 0, 0};
};

// One lane of the wavefront: the dense streams of a slice of a batch, its own
// stream, counters and traversal-stack spill area. A batch is split over the
// lanes and their kernels run concurrently, so one lane's per-bounce launch
// tails (persistent kernels draining) are filled by the other lanes' work;
// only the in-order accumulation is chained lane after lane.
//
// Per path of the slice: the ray streams of two consecutive bounces (ping-
// pong: bounce b reads ray[b & 1], its survivors are appended to
// ray[(b + 1) & 1]), the hit record of bounce b's rays, the shadow stream of
// one bounce, and the radiance (and pixel) at the path's batch index. Nothing
// aliases these buffers: a launch reaches them through its LaunchCtx (below),
// so reallocating a lane's buffers needs no refresh anywhere else.
//
// counts (u32): [0] = bounce 0's ray count (k_generate), then per bounce b a
// 64-bit append counter at u32 index 2 + 2b: low word = rays of bounce b + 1,
// high word = shadow rays emitted at bounce b (k_shade adds both at once).
// Those are the rays the traversal kernels see (the front of a stream). The
// presolved rays of bounce b (wpt_presolve.h; the back of its stream, from the
// slice's last entry downward, with their hit records already written) are
// counted in the 64-bit slot at u32 index kResWord + 2b (low word). Its high
// word counts the rays of bounce b that were resolved to a miss adding nothing
// to their path and dropped (WPT_OPT_DROP_MISS): they are in neither end of
// the stream, so the device reads the low word only; the host adds both.
constexpr int kMaxLanes = 8;  // streams made per session (lanes used: nlanes_)
constexpr uint64_t kMinLanePaths = 1024;  // smaller batches run on one lane
// after the per-bounce words: rays and shadow rays traced by k_finish (the
// path-at-a-time tail of RR-only batches)
constexpr size_t kFinishWord = 2 + 2 * (size_t)kMaxBounces;
constexpr size_t kResWord = kFinishWord + 4;     // k_finish: rays, shadow rays, paths, longest path (bounces)
// after the presolved counts: per bounce b a 64-bit slot at u32 index
// kShResWord + 2b whose low word counts the shadow rays of bounce b that
// k_shade resolved itself (presolve_shadow, WPT_OPT_PRESOLVE_SHADOW): they are
// in no stream, so the device never reads it; the host adds it to the bounce's
// shadow rays. (k_shade reaches it from the append counter: kShResWord - 2
// words past append_ctr(b).)
constexpr size_t kShResWord = kResWord + 2 * ((size_t)kMaxBounces + 1);
// after those: one 64-bit slot whose low word counts the primary rays that
// k_generate_shade resolved and shaded itself (WPT_OPT_GEN_SHADE): they are in
// no stream, so the device never reads it; the host adds it to bounce 0's rays
// and to the presolved rays.
constexpr size_t kGenShadeWord = kShResWord + 2 * ((size_t)kMaxBounces + 1);
constexpr size_t kCountWords = kGenShadeWord + 2;
static_assert(kResWord % 2 == 0 && kShResWord % 2 == 0 && kGenShadeWord % 2 == 0,
              "the presolved counts are 64-bit slots");
constexpr uint32_t kWorkWords = 16;   // device work counters (COUNT builds), see d_work_
constexpr uint32_t kWorkCopies = 64;  // copies of them, one per blockIdx % 64 (spreads the atomics)
struct PathSet {
  hipStream_t stream = nullptr;  // lane 0: the renderer's main stream
  hipStream_t lo = nullptr;      // async batches with WPT_OPT_ASYNC_PRIO: a low-priority stream (lazily made)
  hipEvent_t done = nullptr;     // recorded after the lane's accumulation
  uint64_t cap = 0;
  DevBuf<uint32_t> pixel;        // per path: pixel (round batches: partition pixel index)
  DevBuf<float4> col;            // per path: radiance
  DevBuf<float4> ro[2], rd[2], thr[2];
  // hit records of the two streams (bounce b's at [b & 1]: k_shade(b) reads
  // them while it writes the presolved rays' records of bounce b + 1)
  DevBuf<float> t, t1;
  DevBuf<int32_t> id, id1;
  DevBuf<float4> so, sd, sc;
  DevBuf<uint32_t> counts;    // kCountWords, see above
  PinBuf<uint32_t> h_counts;  // pinned mirror
  DevBuf<uint2> spill;        // traversal-stack spill (entries beyond the LDS slots), spill.cap() entries
  DevBuf<float4> shdir;       // per path: {direction, traced} (k_sh_dirs); grown by SH queries only
  float* hit_t(int k) const { return k ? t1 : t; }
  int32_t* hit_id(int k) const { return k ? id1 : id; }
  // count words: rays of bounce b, shadow rays of bounce b, k_shade's append
  // counter of bounce b
  uint32_t* ext_count(int b) const { return b == 0 ? counts : counts + 2 + 2 * (b - 1); }
  uint32_t* sh_count(int b) const { return counts + 3 + 2 * b; }
  unsigned long long* append_ctr(int b) const { return reinterpret_cast<unsigned long long*>(counts + 2 + 2 * b); }
  // presolved rays of bounce b's stream (k_shade finds them from append_ctr:
  // res_ctr(b + 1) = append_ctr(b) + kResWord / 2)
  unsigned long long* res_ctr(int b) const { return reinterpret_cast<unsigned long long*>(counts + kResWord + 2 * b); }
};

// One batch of the wavefront in flight: its path mapping, its lanes and how
// far its launches are issued. A batch on the main lanes is issued and waited
// for at once (run_batch). An asynchronous batch runs on the async lanes
// (lanes kAsyncLane0 ..) beside the main lanes' work: a refill of the
// adaptive halves' sample stock (wpt_stock.h), or a random half's whole
// rounds under an adaptive half's rounds (the filler); pump() issues it piece
// by piece, because an RR-only batch's launches depend on live counts read
// back every finish_every bounces.
constexpr int kAsyncLane0 = 2;
// The ray source of a query batch (wpt_radiance_rays, wpt_rays.h): a chunk of
// the caller's rays on the device. Position k of the chunk is ray k / spp,
// sample `sample` + k % spp; the ray's sums are entry `ray` of acc / cnt.
struct RayQuery {
  const float* rays = nullptr;     // 6 f32 per ray {ox,oy,oz,dx,dy,dz}
  const uint32_t* keys = nullptr;  // per ray, or null: key0 + ray
  uint32_t key0 = 0;
  uint32_t nrays = 0, spp = 1, sample = 0, type = 0;
  // the query's own accumulation: k_accumulate_round's targets, or for an SH
  // query (sh_nc != 0, wpt_sh.h) the per-record sums, 3 * sh_nc f32 each at entry
  // `ray`, that k_accumulate_sh adds to (cnt is then unused). One slot, so that
  // the struct the generators take by value keeps its size and offsets.
  union {
    float4* acc = nullptr;
    float* sh;
  };
  uint32_t* cnt = nullptr;
  // 0: `rays` are the rays. 1 + dist: they are a point query's records {p, n}
  // (wpt_points.h), the ray of a position made by the generator
  uint32_t source = 0;
  uint32_t sh_nc = 0;  // an SH query: its (order + 1)^2 coefficients per record; else 0 (in the tail padding)
};
static_assert(sizeof(RayQuery) == 64, "the generators' kernarg layout");
// the records of one chunk of an SH query (WPT_SH_CHUNK): its sums are 12 * nc
// bytes per record (108 at order 2) where a ray query's are 20, so 2^18, not 2^21
constexpr size_t kShQueryChunk = (size_t)1 << 18;
constexpr int kQueryVariants = 2;
constexpr int query_variant(bool points) { return points ? 1 : 0; }
struct Batch {
  enum State { kNew, kBouncing, kCountWait, kIssued };
  // positions k0 .. k0+n-1 of: half h's current round (half >= 0), the
  // explicit mapping below (moff != null), or the uniform sequence path k ->
  // (part[k % npix], k / npix)
  uint64_t k0 = 0, n = 0;
  int half = -1;
  const uint32_t* part = nullptr;
  uint32_t npix = 0;
  // explicit mapping (k_generate): entry p covers positions [moff[p],
  // moff[p+1]) with samples mbase[p] ..; entry p is partition entry mlist[p]
  // (or p); a stock batch stores its radiance into the ring
  const uint32_t* moff = nullptr;
  const uint32_t* mbase = nullptr;
  const uint32_t* mlist = nullptr;
  uint32_t nent = 0;
  // a query batch: positions k0 .. k0+n-1 of the rays' chunk (batch_begin then
  // picks the generator pair of the query's source from kGenQueryTable /
  // kGenQueryPsTable, batch_tail the query's sums)
  const RayQuery* rq = nullptr;
  bool stock = false;
  bool async = false;
  int queue = 0;      // async: 0 stock refills, 1 a random half's filler (each its own lanes, in order)
  int lane0 = 0, nl = 1;
  uint64_t off[kMaxLanes + 1] = {};
  bool fused = false, pnee = false;
  bool presolve = false;  // its producers resolve plane-or-miss rays (depth-capped batches on BVH scenes)
  int maxb = 0, b = 0;  // bounce cap, next bounce to issue
  bool finished = false;  // the tail ran as k_finish
  State state = kNew;
  hipEvent_t done[kMaxLanes] = {};  // async: per lane, its slice done
  hipEvent_t live[kMaxLanes] = {};  // async RR-only: the live count landed in hl
  uint32_t* hc = nullptr;           // async: pinned nl x kCountWords, the final counts
  uint32_t* hl = nullptr;           // async: pinned nl live-count words
};

// Where and how one launch runs, passed down to the launchers: made per
// (batch, lane, bounce) by Renderer::batch_ctx, or for lane 0 alone by
// Renderer::lane0_ctx (the test hooks and the photon build).
struct LaunchCtx {
  int lane = 0;
  const PathSet* ps = nullptr;   // lanes_[lane]
  hipStream_t stream = nullptr;  // the lane's, or its low-priority one (async batches with WPT_OPT_ASYNC_PRIO)
  bool async = false;            // the launch belongs to an async batch ...
  uint64_t paths = 0;            // ... of this many paths in the lane's slice
  int batch_lanes = 1;           // lanes of the batch (1: full-capacity traversal grids)
  bool timed = false;            // launch_timed: the main lanes' launches when profiling
  bool count = false;            // the kernels' work-counting variants
  int bounce = 0;
  int hit_sel = 0;               // the hit-record buffers a traversal launch writes (bounce & 1 when presolving)
  // the presolved count of the bounce's stream (probing: added to the
  // launch's record, see k_probe_add), or null
  const uint32_t* probe_res = nullptr;
};

// The numbering of the kernel variants: what a launcher computes from named
// run-time flags, the index into the family's table of instantiations
// (wpt_render.hip, "Kernel variant tables", where each is checked against its
// table) and into the renderer's per-variant grid and occupancy caches.
// k_extend, k_shadow (trav: 0 exact BVH2, 1 BVH4 fast path):
constexpr int trav_variant(bool tri_only, bool count, int trav) {
  return (tri_only ? 1 : 0) | (count ? 2 : 0) | (trav << 2);
}
constexpr int trace_variant(bool tri_only, bool count) { return (tri_only ? 1 : 0) | (count ? 2 : 0); }
// k_shade (oct: the PNEE octree's LDS view, 0 without PNEE; cr: the paths
// write their ray counts; ps: the kernel presolves)
constexpr int shade_variant(bool tri_only, bool pnee, int oct, bool cr, bool ps) {
  return (ps ? 16 : 0) + (cr ? 8 : 0) + (tri_only ? 4 : 0) + (pnee ? 1 + oct : 0);
}
constexpr int finish_variant(bool tri_only, bool pnee, bool cr) {
  return (tri_only ? 1 : 0) | (pnee ? 2 : 0) | (cr ? 4 : 0);
}
// k_generate_shade, k_first_hit, k_first_hit_rays, k_photon_hit
constexpr int scene_variant(bool tri_only) { return tri_only ? 1 : 0; }
// k_photon_sample: the octree view itself
constexpr int oct_variant(int view) { return view; }
constexpr int kTravVariants = trav_variant(true, true, 1) + 1;
constexpr int kTraceVariants = trace_variant(true, true) + 1;
constexpr int kShadeVariants = shade_variant(true, true, 2, true, true) + 1;
constexpr int kFinishVariants = finish_variant(true, true, true) + 1;
constexpr int kSceneVariants = scene_variant(true) + 1;
constexpr int kOctVariants = oct_variant(2) + 1;

// A kernel's resident blocks per CU at one dynamic LDS size, queried on first
// use and again when the size changes (blocks 0: not yet queried).
struct OccCache {
  uint32_t blocks = 0;
  size_t smem = 0;
};

class Renderer {
 public:
  Renderer();
  ~Renderer();
  bool set_device(int dev, std::string& err);
  bool upload_scene(const HostScene& sc, std::string& err);
  bool set_viewport(uint32_t w, uint32_t h, std::string& err);
  void set_camera(const float cam[5]);
  void set_types(int left, int right, int debug) { left_type_ = left; right_type_ = right; debug_ = debug; }
  // AdaptiveSamplingStrategy per screen half (wpt_adaptive.h); takes effect
  // with the next reset
  void set_adaptive(bool left, bool right) { adaptive_[0] = left; adaptive_[1] = right; }
  bool adaptive() const { return adaptive_[0] || adaptive_[1]; }
  // sampling view (results(1), the SimpleRenderTarget): the whole view blue
  // (both strategies' constructors at init, sampling_strategy.rs:42-51,
  // :205-213); reset() clears it and repaints the adaptive halves blue
  bool fill_sampling_blue(std::string& err);
  bool sampling_rgba(uint8_t* out, std::string& err);
  void set_options(int max_depth, uint32_t seed, uint64_t batch) {
    if (seed != seed_) photons_ok_ = false;  // the photon streams derive from the frame seed
    max_depth_ = max_depth; seed_ = seed; if (batch) batch_ = batch;
  }
  // PNEE: shoot photons until kPhotonsNeeded are stored, build + freeze the
  // octree on the host, upload it. Done lazily by compute() when a half of
  // the screen renders PNEE; `photon_tree` exposes the frozen tree.
  bool build_photons(std::string& err);
  // Test hooks. install_photons: a caller's photon list (insertion order) as
  // the session's tree, through build_photons' freeze + upload; whatever
  // drops a shot tree drops it too. Returns -1 for a light id out of range.
  // photon_sample: the device's PhotonTree::sample of n points, each on its
  // own xorshift32 state, reading the tree as k_shade's OCT = `view` variant
  // does (`table` false: no corner table); -1 if the tree does not fit.
  int install_photons(size_t n, const uint32_t* light, const float* loc3, const float* intensity, std::string& err);
  int photon_sample(size_t n, const float* pts3, const uint32_t* states, int view, bool table, uint32_t* light,
                    float* pdf, uint32_t* states_out, std::string& err);
  bool photon_tree(std::vector<uint32_t>& child, std::vector<float>& cum, uint64_t& shot, uint64_t& stored,
                   std::string& err);
  bool set_partition(uint32_t rank, uint32_t nranks, uint32_t tile, std::string& err);
  bool reset(std::string& err);                 // clears accumulation + path counter
  bool compute(uint64_t num_paths, std::string& err);
  bool sync(std::string& err);
  bool results_rgba(uint8_t* host_out, std::string& err);
  bool read_radiance(float* acc3, uint32_t* cnt, std::string& err);
  bool copy_partition(float* dev_dst, std::string& err);   // compact (acc.xyz,cnt) of own pixels
  // Frame exchange of adaptive rounds over several ranks (wpt_set_exchange):
  // fn(user) all-gathers every rank's `slot` float4 at local_dev into
  // gathered_dev (rank-major). exchange_slot() = largest partition.
  using ExchangeFn = int (*)(void*);
  void set_exchange(ExchangeFn fn, void* user, void* local_dev, void* gathered_dev, uint64_t slot) {
    xfn_ = fn; xuser_ = user; xlocal_ = (float4*)local_dev; xall_ = (float4*)gathered_dev; xslot_ = slot;
  }
  uint64_t exchange_slot() const { return maxpart_; }
  uint32_t rank() const { return rank_; }
  uint32_t nranks() const { return nranks_; }
  uint32_t tile() const { return tile_; }
  bool unpack_ranks(const float4* gathered, uint64_t slot, std::string& err);
  bool trace_rays(size_t n, const float* rays, float* t_out, int32_t* id_out, std::string& err);
  // first-hit feature planes of sample `sample` of every frame pixel
  // (wpt_first_hit, include/wpt.h); a null plane is not computed
  bool first_hit(uint32_t sample, float* dir3, float* t, int32_t* id, uint32_t* visits, float* normal3,
                 float* albedo3, uint8_t* kind, std::string& err);
  // the same planes for the virtual viewport scale * width x scale * height
  // under the session's camera and seed (wpt_first_hit_scaled), in a buffer of
  // its own: first_hit's, which the filter, the reprojection and the sample map
  // leave their guides in, is not written. The caller checks scale (0 here is
  // first_hit itself: the session's viewport, first_hit's buffer).
  bool first_hit_scaled(uint32_t scale, uint32_t sample, float* dir3, float* t, int32_t* id, uint32_t* visits,
                        float* normal3, float* albedo3, uint8_t* kind, std::string& err);
  // guided upsampling (wpt_upsample.h) of the session's frame, or with
  // kUpMerged of the last reproject's merged frame (the caller checks
  // has_merged()), to scale times the viewport: the filter's pack and passes at
  // the session viewport, then k_upsample under the fine first-hit planes of
  // `sample`; a null output is not written
  bool upsample(uint32_t scale, uint32_t sample, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags,
                float* rgb3, uint8_t* valid, uint8_t* rgba, std::string& err);
  // the a-trous filter (wpt_denoise.h) on the session's frame, guided by the
  // first-hit planes of `sample` (wpt_denoise); a null output is not written
  bool denoise(uint32_t sample, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags, float* rgb3,
               uint8_t* valid, uint8_t* rgba, std::string& err);
  // reverse reprojection of the kept history into the current camera, merged
  // with the session's frame (wpt_reproject.h, wpt_reproject); a null output is
  // not written. keep: the merged frame, the planes of `sample` and the camera
  // become the history. The caller checks history_state() != 2 first.
  bool reproject(uint32_t sample, float cos_min, float eps_z, uint32_t max_len, uint32_t flags, float* acc3,
                 uint32_t* cnt, uint32_t* len, std::string& err);
  // the a-trous filter over the merged frame and the guide planes the last
  // reproject of this viewport left on the device (wpt_denoise_merged)
  bool has_merged() const { return post_.has_merged(); }
  bool denoise_merged(uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags, float* rgb3, uint8_t* valid,
                      uint8_t* rgba, std::string& err);
  // WPT_OPT_HISTORY: 0 no history, 1 usable, 2 kept in the current accumulation
  int history_state() const { return post_.history_state(epoch_); }
  void history_drop() { post_.history_drop(); }
  // Guided sampling (wpt_guided.h). sample_map: the map planned from the
  // counts, the len plane of this accumulation's last reproject and (under
  // WPT_MAP_MISS_ONCE) the first-hit kinds of `sample`; it stays on the device
  // for compute_map(nullptr). compute_map: pixel p of the partition gets
  // count[p] samples from sample cnt[p] on. `invalid`: the failure is the
  // caller's argument (WPT_ERR_INVALID_ARG), nothing was traced or kept.
  bool sample_map(uint32_t sample, uint32_t target, uint32_t max_pp, uint32_t budget, uint32_t flags,
                  uint32_t* count_out, uint64_t* total_out, bool& invalid, std::string& err);
  bool compute_map(const uint32_t* count, bool& invalid, std::string& err);
  // Radiance along a caller's rays (wpt_rays.h, wpt_radiance_rays): camera paths
  // of render type `type` whose primary rays are rays6, samples sample ..
  // sample + spp - 1 on the streams of keys (null: the ray's index), summed per
  // ray in sample order into rgb3; status (may be null) 0 for a ray not traced.
  // device: the four are device pointers. The batches are run_batch's with the
  // rays as their source; the frame, the rounds, the stock and the map are not
  // touched. The caller checks the arguments.
  bool radiance_rays(size_t n, const float* rays6, const uint32_t* keys, uint32_t sample, uint32_t spp, uint32_t type,
                     bool device, float* rgb3, uint8_t* status, std::string& err);
  // Hemisphere gathers at a caller's points (wpt_points.h, wpt_radiance_points):
  // radiance_rays with the records {p, n} as the source and the generators of
  // dist (kPointsCosine / kPointsSphere) making each position's ray.
  bool radiance_points(size_t n, const float* points6, const uint32_t* keys, uint32_t sample, uint32_t spp,
                       uint32_t type, uint32_t dist, bool device, float* rgb3, uint8_t* status, std::string& err);
  // SH projection of a point's gathers (wpt_sh.h, wpt_probe_sh): radiance_points
  // whose samples are weighted by the SH basis of their own directions; sh holds
  // 3 * (order + 1)^2 f32 per record.
  bool probe_sh(size_t n, const float* points6, const uint32_t* keys, uint32_t sample, uint32_t spp, uint32_t type,
                uint32_t dist, uint32_t order, bool device, float* sh, uint8_t* status, std::string& err);
  // first_hit's planes along a caller's rays (wpt_first_hit_rays.h,
  // wpt_first_hit_rays): entry i is what first_hit gives a pixel whose primary
  // ray is rays6[i]; status as radiance_rays gives it; a null plane is neither
  // computed nor stored. device: every pointer is a device pointer. Needs a
  // scene, no viewport; works in d_fhr_, so first_hit's buffers, which keep the
  // guides of the filter, the reprojection and the sample map, the frame, the
  // rounds, the counters and the timings are neither read nor written. Host
  // rays go through in chunks of kQueryChunk. The caller checks the arguments.
  bool first_hit_rays(size_t n, const float* rays6, bool device, float* t, int32_t* id, uint32_t* visits,
                      float* normal3, float* albedo3, uint8_t* kind, uint8_t* status, std::string& err);
  // The a-trous filter on a W x H frame of a caller's rays (wpt_denoise_rays):
  // radiance_rays' sums of the rays (raw3, status), first_hit_rays' guide planes
  // of the same rays and post_.denoise over both with cnt = spp * status; the
  // sums, the counts, the planes and the filter's scratch stay on the device
  // (d_rayframe_, one frame whatever the query's chunks). The session is left
  // as radiance_rays leaves it. A null output is not written; with all five
  // null nothing is launched. The caller checks the arguments.
  bool denoise_rays(uint32_t W, uint32_t H, const float* rays6, const uint32_t* keys, uint32_t sample, uint32_t spp,
                    uint32_t type, const DnParams& P, bool device, float* rgb3, uint8_t* valid, uint8_t* rgba,
                    float* raw3, uint8_t* status, std::string& err);
  // WPT_OPT_MAP_MODE: a map was traced in this accumulation (wpt_compute is an
  // error until the next reset)
  bool map_mode() const { return map_mode_; }
  // test hook: presolve_ray on the device over caller-given rays
  bool presolve_rays(size_t n, const float* rays, uint8_t* resolved, float* t_out, int32_t* id_out, std::string& err);
  // test hook: presolve_shadow on the device over caller-given {p, q} pairs
  bool presolve_shadow_rays(size_t n, const float* pq, const int32_t* light, uint8_t* resolved, std::string& err);
  bool shadow_rays(size_t n, const float* pq, const int32_t* light, uint8_t* occ, std::string& err);
  // the recorded wave timelines (WPT_OPT_PROBE), then recording restarts
  bool probe_read(std::vector<uint32_t>& meta, std::vector<uint4>& rec, double& ticks_per_us, std::string& err);
  void set_counting(bool on) { counting_ = on; }
  void set_profiling(bool on) { profiling_ = on; }
  // concurrent lanes of the next batches (1..the count made at set_device);
  // one lane serialises the kernels (their standalone times)
  bool set_lanes(int n) {
    if (n < 1 || n > lanes_made_) return false;
    nlanes_ = n;
    return true;
  }
  int lanes() const { return nlanes_; }
  // true if `opt` shapes the device scene (re-uploaded when it changes)
  static bool scene_option(int opt) { return opt == 1 || opt == 2 || opt == 10; }
  // Launch configuration (wpt_set_option, include/wpt.h WPT_OPT_*). No
  // environment variable changes it: the defaults below are the measured
  // production settings. Options that shape the device scene
  // (traversal, treelet) take effect at the next upload_scene, the pixel tile
  // at the next set_partition; the caller (wpt_api.cpp) re-runs those.
  bool set_option(int opt, int64_t v, std::string& err);
  bool get_option(int opt, int64_t& v) const;
  // the scene build's BVH4 collapse (HostScene::want_bvh4): 1 always
  // (traversal bvh4), 2 for scenes with other shapes than triangles (auto)
  int wants_bvh4() const {
    return (traversal_ == 1 || traversal_sh_ == 1) ? 1 : (traversal_ == 3 || traversal_sh_ == 3) ? 2 : 0;
  }
  // the adaptive rounds' sum path on host data (tests): chunk effects on the
  // device, the walk on the host
  bool seq_sum_device(const float* v, uint64_t n, float& out, std::string& err);
  // Test hooks: the two parts of plan_round (estimate_errors, plan_counts) on
  // a host frame of W x H pixels, in scratch buffers; the session's frame,
  // rounds and stock are not touched.
  bool adaptive_error(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, int half, float* mse_out,
                      float* stats3, std::string& err);
  bool adaptive_plan(uint32_t W, uint32_t H, int half, bool first, bool adaptive, const float* mse,
                     const float* stats3, const uint32_t* cnt, uint32_t* count, uint32_t* offset, uint32_t* base,
                     uint8_t* samp, std::string& err);
  const Stats& stats() const { return stats_; }
  const KernelTimes& times() const { return times_; }
  void clear_stats() {
    std::string e;
    (void)flush_counts(e);  // a batch still in flight must not land in the cleared counters
    stats_ = Stats();
    times_ = KernelTimes();
  }
  bool flush_counts(std::string& err);  // the last batch's per-lane counts into stats_ (waits for them)
  uint32_t width() const { return w_; }
  uint32_t height() const { return h_; }
  uint32_t part_pixels() const { return (uint32_t)part_pix_.size(); }
  const std::vector<uint32_t>& part_list() const { return part_pix_; }
  hipStream_t stream() const { return stream_; }
  // the frame post-processing; its *_planes test hooks need stream() and nothing else of the session
  FramePost& post() { return post_; }
  uint32_t bvh_depth() const { return depth_; }

 private:
  bool ensure_paths(uint64_t n, std::string& err);   // lane 0 holds >= n paths
  bool ensure_lane(int i, uint64_t n, std::string& err);
  void free_lane_paths(PathSet& L);
  LaunchCtx batch_ctx(const Batch& B, int i, int b) const;  // slice i of B at bounce b
  LaunchCtx lane0_ctx(bool count) const;                     // lane 0 alone, untimed
  // half < 0: progressive paths k0.. over the partition; half 0/1: positions
  // k0.. of that screen half's current sample round
  bool run_batch(uint64_t k0, uint64_t n, int half, std::string& err, const uint32_t* part_pix = nullptr,
                 uint32_t part_n = 0, const Batch* map = nullptr);
  // the Batch state machine: lanes and generate; bounces until done or a
  // live-count read is pending (block: wait for it); the tail
  auto shade_params() const;  // the ShadeParams of a batch's shade kernels (wpt_render.hip)
  // the GenParams of a mapping over npix entries, for the viewport scale * w_ x scale * h_ (wpt_render.hip)
  auto gen_params(uint32_t npix, uint32_t scale = 1) const;
  bool batch_begin(Batch& B, std::string& err);
  bool batch_advance(Batch& B, bool block, std::string& err);
  bool batch_tail(Batch& B, std::string& err);
  void batch_counts(const Batch& B, const uint32_t* hc);  // a finished async batch's counts into stats_
  // async lanes: issue queued batches as far as they go (block: the head to
  // its end); wait until one is issued; issue and wait for all of them
  bool pump(bool block, std::string& err);
  bool wait_issued(Batch* B, std::string& err);
  bool drain_async(std::string& err);
  bool host_wait(hipEvent_t e, std::string& err);          // pumps the async lanes while it waits
  bool host_wait_stream(hipStream_t s, std::string& err);
  hipEvent_t ev_sync_ = nullptr;
  uint64_t batch_cap() const;
  int main_lanes() const;  // lanes of main batches (below the async lanes in adaptive sessions)
  bool compute_half(int h, uint64_t n, std::string& err);
  bool merge_random_halves(uint64_t nl, uint64_t nr, bool& merged, std::string& err);
  bool plan_round(int h, std::string& err);
  // plan_round's buffers and its two parts, which the wpt_adaptive_* hooks
  // run on frames of their own: element counts of the buffers (one formula
  // for both), a half's error estimate, the round's counts and offsets
  struct RoundSizes {
    size_t scan_sums;  // block sums of the offsets' scan (+ 1)
    size_t mse;        // a half's errors, then the {min, max} keys
    size_t bmm;        // per-tile {min, max} keys
    size_t chunks;     // chunks of the errors' sum (+ 1)
    size_t fetch;      // packed elements of the chunks the walk re-sums
  };
  static RoundSizes round_sizes(uint32_t w, uint32_t h, uint32_t pn);
  struct ErrorBufs {
    float *d_mse, *h_mse;
    uint32_t* d_bmm;
    double* d_s64;
    ChunkEff *d_eff, *h_eff;
    uint32_t *d_need, *d_list, *h_list;
    float *d_fb, *h_fb;
  };
  bool estimate_errors(const float4* acc, const uint32_t* cnt_px, uint32_t W, uint32_t H, int h, const ErrorBufs& B,
                       float stats[3], std::string& err);
  bool plan_counts(uint32_t W, uint32_t H, uint32_t pn, int h, bool adaptive, bool first, const float stats[3],
                   const uint32_t* cnt_px, const float* mse_l, const float* mse_r, uint32_t* rc, uint32_t* rbase,
                   uint32_t* sums, uint8_t* samp, uint32_t* h_total, std::string& err);
  bool exchange_frame(std::string& err);
  bool plan_slice(int h, uint64_t a, uint64_t b, uint64_t& local, std::string& err);
  void free_rounds();
  // The launchers: each takes its kernel's variant from the session's and the
  // batch's state (wpt_render.hip, "Kernel variant tables") and launches it in
  // context C. launch_timed runs `launch` (one kernel launch) and, when C is
  // timed, records its interval for timing slot `slot` (resolve_timings).
  template <class F>
  bool launch_timed(const LaunchCtx& C, int slot, F&& launch, std::string& err);
  bool launch_generate(const Batch& B, int i, std::string& err);  // bounce 0 of slice i
  bool launch_shade(const Batch& B, const LaunchCtx& C, std::string& err);
  // the live paths of C's lane after bounce C.bounce, to their end (g blocks)
  bool launch_finish(const Batch& B, const LaunchCtx& C, uint32_t g, std::string& err);
  bool launch_extend(const LaunchCtx& C, const float4* ro, const float4* rd, const uint32_t* cnt, std::string& err);
  bool launch_shadow(const LaunchCtx& C, const uint32_t* cnt, uint8_t* occ_out, std::string& err);
  bool launch_trace(const LaunchCtx& C, std::string& err);
  bool size_grids(std::string& err);
  uint32_t max_grid() const;
  size_t spill_slots() const;
  uint32_t spill_grid(const PathSet& L) const;
  bool ensure_spill(int l, uint32_t grid, std::string& err);
  // one-shot grid of a slice of `paths` (fused: 2 rays per path), its spill
  // area capped at 1 GiB (beyond it the grid is clamped: partly persistent)
  uint32_t oneshot_grid(uint64_t paths) const {
    const uint64_t g = (2 * paths + 255) / 256;
    const uint64_t gmax = (1ull << 30) / (sizeof(uint2) * 256 * spill_slots());
    return (uint32_t)std::max<uint64_t>(1, std::min(g, gmax));
  }
  void free_scene();
  void free_paths();
  void free_photons();
  void free_frame();       // the viewport's frame buffers and the scaled first-hit planes
  void free_partition();   // the pixel lists, the exchange index, compute_map's plan
  void free_stock_side();  // the ring's side buffers and the refill pool (not the ring)
  bool upload_photons(const PhotonTree& tree, std::string& err);
  // Sample rounds, per screen half: as the reference's two RenderInstances
  // (wasm_interface.rs:90-94, :374-379), each half has its own strategy and
  // its own sequence of sample positions, and compute(n) advances the left
  // half's sequence by n/2 and the right half's by n - n/2. An adaptive half's
  // rounds are AdaptiveSamplingStrategy's (wpt_adaptive.h); a random half's
  // round gives each of its pixels one sample.
  bool adaptive_[2] = {false, false};
  struct HalfRounds {
    uint64_t total = 0, pos = 0;    // positions in the current round / taken
    uint32_t idx = 0;               // rounds planned since the reset
    DevBuf<uint32_t> rc;            // samples per partition pixel -> (scan) offsets, [npix] = total
    DevBuf<uint32_t> rbase;         // samples of the pixel before the round
    // several ranks: the round is planned over the whole frame (global
    // offsets gc, bases gbase); rc / rbase then hold this rank's slice
    DevBuf<uint32_t> gc, gbase;
  } rounds_[2];
  uint64_t round_cap_ = 0;
  DevBuf<uint32_t> d_scan_sums_, d_gsums_;
  DevBuf<float> d_mse_[2];
  DevBuf<uint32_t> d_bmm_;          // per-tile {min, max} error keys of a half
  PinBuf<float> h_mse_[2];          // pinned copies of the per-pixel errors (host sum)
  // the errors' sequential sum: per-chunk f64 sums / prefixes and chunk
  // effects on the device (k_sum_*), the effects' pinned copy for the walk
  DevBuf<double> d_s64_;
  DevBuf<ChunkEff> d_eff_;
  PinBuf<ChunkEff> h_eff_;
  DevBuf<uint32_t> d_need_;       // per chunk: the walk will likely re-sum it
  DevBuf<uint32_t> d_list_;       // those chunks: count, then their indices
  DevBuf<float> d_fb_;            // the elements of the first kSumFetch of them
  PinBuf<uint32_t> h_list_;
  PinBuf<float> h_fb_;
  // The sample stock of adaptive halves (wpt_stock.h, WPT_OPT_STOCK): a ring
  // of stock_slots_ samples per pixel of this rank's partition (radiance +
  // ray counts) and the id of the refill tracing each, the frontier per
  // partition entry, the consumed rays and samples; the refills in flight (a
  // pool; each one async batch on one stock lane, in turn); the round's
  // deficit offsets. With several ranks (WPT_OPT_STOCK_RANKS) the rounds are
  // the global ones every rank plans; a rank stocks its own pixels only.
  uint32_t stock_slots_ = 1024;  // WPT_OPT_STOCK (power of two; 0: off): at most, see stock_alloc
  int stock_lanes_ = 2;         // WPT_OPT_STOCK_LANES: async lanes the refills rotate over
  uint32_t stock_ahead_ = 40;   // WPT_OPT_STOCK_AHEAD: a refill stocks ahead * c + extra samples per pixel
                                // (40 vs 24 at a refill every 3 rounds: C5 +2.7 %, init defaults equal,
                                // profiles/r06/ab_stock_ahead40_*.jsonl)
  uint32_t stock_extra_ = 8;    // WPT_OPT_STOCK_EXTRA
  uint32_t stock_every_ = 3;    // WPT_OPT_STOCK_EVERY: a refill after every this many rounds of a half
                                // (3 vs 2: C5 +1.3 %, init defaults +0.4 %, profiles/r06/ab_stock_every3.jsonl)
  // the ring pair stays raw: ring_take / ring_give own it across sessions
  float4* d_stock_ = nullptr;
  uint32_t* d_stock_id_ = nullptr;
  size_t stock_bytes_[2] = {0, 0};   // the two ring blocks' sizes (cached blocks may be larger)
  DevBuf<uint32_t> d_front_;
  DevBuf<uint32_t> d_def_;           // [npart + 1] deficit counts -> offsets, then [npart] bases
  DevBuf<uint32_t> d_bmax_;          // per-block maxima scratch
  DevBuf<unsigned long long> d_rays_;     // [3] consumed rays (extension, shadow) and samples, [1] unused, + scratch
  uint64_t stock_cap_ = 0;           // partition pixels x slots the ring holds (0: not allocated)
  uint64_t stock_frame_ = 0;         // the viewport's pixels when the ring was made (a resize orphans it)
  uint32_t stock_used_slots_ = 0;
  static constexpr int kMaxRefill = 8;
  static constexpr uint64_t kStockBytes = 48ull << 30;  // the ring's HBM at most (1080p: 1024 slots, 42 GB)
  static constexpr int kRefillChunks = 8;                 // async batches of one refill (at most)
  static constexpr uint64_t kRefillChunk = 1ull << 25;    // paths per batch
  struct Refill {
    uint32_t id = 0;
    bool live = false;
    bool counted = false;      // its batches' counts are in stats_ (stock_rays, bounces)
    DevBuf<uint32_t> off;      // [n + 1] counts -> offsets over the half's list
    DevBuf<uint32_t> base;     // [n] first sample per pixel
    std::deque<Batch> chunks;  // its batches (stable addresses: the queue points at them)
  };
  Refill refills_[kMaxRefill];
  hipEvent_t refill_ev_[kMaxRefill][2 * kRefillChunks] = {};
  PinBuf<uint32_t> h_refill_cnt_;     // pinned [kMaxRefill][kRefillChunks][kCountWords + 1]
  uint32_t refill_id_ = 0;            // ids of the session's refills, in issue order
  int refill_lane_ = 0;               // the stock lane of the next refill
  uint32_t round_need_[2] = {0, 0};   // per half: 1 + the refill its current round's samples wait for (0: none)
  bool stock_redo_[2] = {false, false};  // per half: the stock was dropped while its round was partly added
  int log_ = 0;  // WPT_OPT_LOG: host steps of the adaptive rounds and async lanes to stderr (debugging)
  // WPT_OPT_STOCK_RANKS: sessions with several ranks use the stock. Off by
  // default: the only measurement so far, two ranks sharing one card, read
  // 892-976 Mray/s with it and 751-955 without, ranges that overlap
  // (profiles/stockranks/README.md)
  bool stock_ranks_ = false;
  // half h's rounds take their samples from the stock; with several ranks a
  // rank that owns no pixel of the half has nothing to stock
  bool stock_active(int h) const {
    return stock_slots_ != 0 && adaptive_[h] && (nranks_ == 1 || (stock_ranks_ && half_npix_[h] != 0));
  }
  // the session runs async lanes (refills, the filler) beside its main lanes
  bool async_lanes() const {
    return ((stock_slots_ && (nranks_ == 1 || stock_ranks_)) || (fill_on_ && nranks_ == 1)) &&
           (adaptive_[0] || adaptive_[1]);
  }
  // WPT_OPT_STOCK_RING_BYTES: the ring's two blocks (float4 + refill id per
  // slot) as the session sized them; a cached block reused for one may be
  // larger. A ring the session stopped using (the stock switched off, another
  // partition) is held, and counted, until the next ring is sized
  uint64_t ring_bytes() const { return d_stock_ ? stock_cap_ * (sizeof(float4) + sizeof(uint32_t)) : 0; }
  bool stock_alloc(std::string& err);
  void stock_drop();                     // forget the ring (reset, reallocation)
  bool stock_round(int h, uint64_t left, std::string& err);   // after half h's round is planned: deficit + refill
  bool stock_consume(int h, uint64_t a, uint64_t b, std::string& err);
  bool stock_flush(std::string& err);    // consumed rays into stats_, finished refills' counts
  bool refill_count(Refill& f, bool block, std::string& err);
  uint32_t refill_scale(int h, uint32_t ahead, uint64_t after) const;
  Refill* refill_slot(std::string& err);
  void refill_plan(Refill& F, int h, uint32_t ahead, uint32_t q);
  bool refill_issue(Refill& F, int h, uint64_t wt, std::string& err);
  bool stock_prefill(int h, uint64_t budget, std::string& err);  // at a compute call's start
  bool stock_prefill_ = true;  // WPT_OPT_STOCK_PREFILL
  std::deque<Batch*> aq_[2];  // per queue: async batches not yet fully issued, in order
  // A random half's whole rounds traced beside the adaptive half's rounds
  // (WPT_OPT_FILL, compute_halves): its pixels outside the seam (the two
  // columns the other half's 5x5 error filter reads, render_target.rs:112-128)
  // run on the fill lane; the seam columns on the main lanes.
  bool fill_on_ = false;  // measured slower than tracing the random half on the main lanes with the stock on (profiles/r06)
  int async_prio_ = 0;       // WPT_OPT_ASYNC_PRIO: async batches on low-priority streams
  // the async batches (stock refills) run the fused k_trace up to 2^26 paths
  // on grids of the whole resident capacity: C5 +1.4 %, init defaults +1.9 %
  // same-session (profiles/r06/ab_async_fused_grid.jsonl)
  int async_grid_pct_ = 100;  // WPT_OPT_ASYNC_GRID_PCT: their traversal grids, % of resident capacity (0: the main batches')
  uint64_t async_fused_below_ = 1ull << 26;  // WPT_OPT_ASYNC_FUSED_BELOW: async batches below this many paths run fused (0: fused_below)
  DevBuf<uint32_t> d_seam_pix_[2], d_rest_pix_[2];
  uint32_t seam_npix_[2] = {0, 0}, rest_npix_[2] = {0, 0};
  static constexpr int kMaxFill = 8;
  Batch fill_[kMaxFill];
  int nfill_ = 0;
  hipEvent_t fill_ev_[kMaxFill][2] = {};
  PinBuf<uint32_t> h_fill_cnt_;     // pinned [kMaxFill][kCountWords + 1]
  bool async_pending() const { return !aq_[0].empty() || !aq_[1].empty(); }
  int fill_lane() const { return kAsyncLane0 + stock_lanes_; }
  bool issue_fill(int h, uint64_t k0, uint64_t n, std::string& err);
  bool drain_fill(std::string& err);
  bool compute_halves(uint64_t nl, uint64_t nr, std::string& err);
  // the traversal grid of a launch: the main batches' persistent grid g (of
  // base_pct % of the resident capacity); for an async batch a share of it
  // (WPT_OPT_ASYNC_GRID_PCT), or with WPT_OPT_ASYNC_ONESHOT one block per
  // kTBlock of the most rays the launch can see (rays_per_path x the slice):
  // every wave takes at most one feed chunk, so its blocks retire as soon
  // as their rays end and free the CUs for the main lanes' next kernel
  uint32_t async_grid(const LaunchCtx& C, uint32_t g, int base_pct, uint32_t rays_per_path = 1) const {
    if (!C.async) return g;
    if (async_oneshot_) return std::max<uint32_t>(1u, (uint32_t)((C.paths * rays_per_path + 255) / 256));
    return async_grid_pct_ > 0 ? std::max<uint32_t>(1u, (uint32_t)((uint64_t)g * async_grid_pct_ / base_pct)) : g;
  }
  bool async_oneshot_ = false;  // WPT_OPT_ASYNC_ONESHOT
  DevBuf<uint8_t> d_samp_;          // sampling visualisation RGBA8 (allocated with the viewport)
  ExchangeFn xfn_ = nullptr;
  void* xuser_ = nullptr;
  float4* xlocal_ = nullptr;
  float4* xall_ = nullptr;
  uint64_t xslot_ = 0;
  uint64_t maxpart_ = 0;             // largest partition over all ranks
  DevBuf<uint32_t> d_xidx_;          // gathered entry -> pixel (~0: padding), nranks * maxpart_
  bool photons_ok_ = false;
  uint64_t photons_shot_ = 0, photons_stored_ = 0;
  std::vector<uint32_t> oct_child_;
  std::vector<float> oct_cum_;
  DevBuf<uint32_t> d_oct_child_;
  DevBuf<float> d_oct_cum_;
  DevBuf<uint32_t> d_oct_corners_;

  int device_ = -1;
  int ncu_ = 256;
  // persistent grids per kernel variant (trav_variant): [v] multi-lane
  // batches (grid_pct_ of the resident capacity), [kTravVariants + v]
  // one-lane batches (all of it); k_trace: trace_variant
  uint32_t grid_ext_[2 * kTravVariants] = {};
  uint32_t grid_sh_[2 * kTravVariants] = {};
  uint32_t grid_tr_[kTraceVariants] = {};
  uint32_t grid_shade_ = 512;      // k_shade blocks (kShadeBlock lanes each) resident on the chip (the least occupied variant)
  OccCache shade_occ_[kShadeVariants];  // per shade_variant
  bool fused_ = false;             // WPT_OPT_FUSED: bounce b's extension + bounce b-1's shadow rays in one k_trace for every batch
  // batches below this many paths (adaptive sample rounds) always run fused:
  // one launch per bounce drains one pool of rays instead of two (WPT_OPT_FUSED_BELOW)
  uint64_t fused_below_ = 1ull << 24;
  int small_lanes_ = 2;           // WPT_OPT_SMALL_LANES: lane cap for batches below fused_below_ (C5 +3-4 %, init defaults +1 % vs 3)
  int traversal_ = 3, traversal_sh_ = 3;  // WPT_OPT_TRAVERSAL(_SH): 0 exact BVH2, 1 BVH4 fast path, 3 auto (per scene)
  int trav_ext_ = 0, trav_sh_ = 0;        // what the uploaded scene runs (0 the exact BVH2, 1 the BVH4 fast path)
  bool treelet_ = true;            // WPT_OPT_TREELET: LDS treelet of the BVH2's top node pairs
  // WPT_OPT_PIXEL_TILE: whole-round batches in tiles of this many px (0: raster);
  // 4 x 4 vs 8 x 8 is within noise (profiles/r06/ab_pixel_tile.jsonl)
  uint32_t pixel_tile_ = 8;
  int grid_pct_ = 50;              // WPT_OPT_GRID_PCT: persistent traversal grids of multi-lane batches, % of resident capacity
#ifndef WPT_TRACE_GRID_PCT
#define WPT_TRACE_GRID_PCT 75  // C5 +0.6 % over 100 (profiles/r05/ab_trace_grid75.jsonl)
#endif
  int trace_grid_pct_ = WPT_TRACE_GRID_PCT;  // WPT_OPT_TRACE_GRID_PCT: the same for the fused k_trace (small batches)
  uint32_t refill_ = 12, refill_sh_ = 16;  // WPT_OPT_REFILL(_SH): idle lanes before a wave refills
  uint64_t finish_below_ = 1u << 18;  // WPT_OPT_FINISH_BELOW: RR-only batches hand their last paths to k_finish (0: never)
  int finish_every_ = 4;           // WPT_OPT_FINISH_EVERY: bounces between the RR-only batches' live-count reads
  uint32_t num_guards_ = 0;        // the uploaded scene's guard boxes (0: its rays are never presolved)
  uint32_t light_guards_ = 0;      // its light guards (bit mask; 0: k_shade does not try to resolve shadow rays)
  bool presolve_ = true;           // WPT_OPT_PRESOLVE: producers resolve plane-or-miss extension rays (wpt_presolve.h)
  bool drop_miss_ = true;          // WPT_OPT_DROP_MISS: a ray resolved to a miss that adds nothing is not written to the next stream
  bool presolve_shadow_ = true;    // WPT_OPT_PRESOLVE_SHADOW: k_shade adds the contribution of a shadow ray it resolves unoccluded
  bool gen_shade_ = true;          // WPT_OPT_GEN_SHADE: k_generate_shade shades the primary rays it resolves (bounce 0 of them in no stream)
  OccCache gen_shade_occ_[kSceneVariants];  // k_generate_shade, per scene_variant
  // WPT_OPT_PROBE: wave timelines of the next probe_cap_ traversal launches
  // (probe_read); meta per launch {kernel, lane, bounce, waves, first entry}
  uint32_t probe_cap_ = 0, probe_waves_ = 0, probe_used_ = 0;
  DevBuf<uint4> d_probe_;
  std::vector<uint32_t> probe_meta_;
  uint4* probe_slot(const LaunchCtx& C, int kernel, uint32_t grid);
  DevBuf<uint32_t> d_fallback_;    // [2] rays re-traced exactly (extend, shadow)
  // first_hit's own buffers, kept between calls: the overflow flag and the
  // planes; the traversal-stack spill area of its grid
  DevBuf<char> d_fh_;
  DevBuf<uint2> d_fh_spill_;
  // k_first_hit of the planes in `mask` into d_fh_; waits for it. scale != 0:
  // the virtual viewport scale * w_ x scale * h_, into d_fhs_ (first_hit_scaled,
  // upsample's fine guides; made on first use, freed with the viewport).
  struct FhPlanes : Guides {
    const uint32_t* visits = nullptr;
  };
  bool first_hit_launch(uint32_t sample, uint32_t mask, FhPlanes& planes, std::string& err, uint32_t scale = 0);
  DevBuf<char> d_fhs_;
  // The filter, the reprojection, the upsampling and the sample map's planning
  // with the state they keep between calls (wpt_post.h). post_ knows nothing of
  // the session: frame_ref() is what it is told of the frame. epoch_ counts the
  // resets of the accumulation (reset() is the one place each passes through).
  FramePost post_;
  FrameRef frame_ref() const { return FrameRef{w_, h_, d_acc_, d_cnt_, cam_, ds_.bg, epoch_, stream_}; }
  uint64_t epoch_ = 0;
  // compute_map's uploaded map, offsets, bases, scan sums and words (freed with
  // the partition). map_mode_: reset() clears it.
  DevBuf<char> d_mplan_;
  bool map_mode_ = false;
  // radiance_rays' scratch of one chunk of rays (sums, counts; for host pointers
  // also rays, keys, rgb, status) and its pinned staging block; freed with the
  // lanes
  DevBuf<char> d_query_;
  PinBuf<char> h_query_;
  // The chunks of a query: radiance_rays' body. sums / cnts non-null: the n
  // rays' float4 sums and counts go there (device, entry i = ray i: one frame
  // over all chunks; rays6, keys, rgb3 and status are then device pointers)
  // and rgb3 may be null: no packed copy is made. source: RayQuery::source.
  // sh_nc > 0: an SH query of that many coefficients (chunks of kShQueryChunk
  // records); rgb3 is then its output, 3 * sh_nc f32 per record.
  bool query_chunks(size_t n, const float* rays6, const uint32_t* keys, uint32_t sample, uint32_t spp, uint32_t type,
                    bool device, float* rgb3, uint8_t* status, float4* sums, uint32_t* cnts, std::string& err,
                    uint32_t source = 0, uint32_t sh_nc = 0);
  // first_hit_rays' own buffers, kept between calls and freed with first_hit's:
  // the overflow flag, then for host pointers a chunk's rays, planes and status;
  // the traversal-stack spill area of its grid
  DevBuf<char> d_fhr_;
  DevBuf<uint2> d_fhr_spill_;
  struct FhrPlanes {  // device pointers; a plane outside the launch's mask is not looked at
    float* t = nullptr;
    int32_t* id = nullptr;
    uint32_t* visits = nullptr;
    float* normal = nullptr;
    float* albedo = nullptr;
    uint8_t* kind = nullptr;
  };
  // k_first_hit_rays of the planes in `mask` over n device rays into P; returns
  // once the kernel has ended without a stack overflow
  bool first_hit_rays_launch(uint32_t n, const float* d_rays, uint32_t mask, const FhrPlanes& P, std::string& err);
  // denoise_rays' frame: the sums, the counts, the guide planes and the status
  // of every ray, for host pointers also the rays, the keys and the packed
  // sums; freed with the lanes
  DevBuf<char> d_rayframe_;
  bool compute_end(std::string& err);  // what every tracing call ends with: counts, overflow flag, work counters
  hipStream_t stream_ = nullptr;
  PathSet lanes_[kMaxLanes];
  int lanes_made_ = 0;
  // the last main batch, until flush_counts reads its counts: its lanes and
  // bounces; it traced stock samples (its rays count when consumed); it
  // presolved (its presolved counts were cleared and copied)
  bool stats_pending_ = false;
  int pend_nl_ = 0, pend_b_ = 0;
  bool pend_stock_ = false, pend_presolve_ = false;
  int nlanes_ = 4;                 // wpt_set_lanes (1..kMaxLanes); 4 with half-GPU traversal grids (C3 +4.5 % over 3 lanes at full grids)
  hipEvent_t ev_main_ = nullptr;   // lanes > 0 wait for the main stream's prior work
  hipEvent_t ev_ref_ = nullptr;    // profiling: time origin of a batch's launch intervals
  std::vector<DevBuf<char>> scene_bufs_;
  DevScene ds_{};
  uint32_t depth_ = 0;
  bool scene_ok_ = false;

  uint32_t w_ = 0, h_ = 0;
  float cam_[5] = {0, 0, 0, 0, 0};
  int left_type_ = 1, right_type_ = 1, debug_ = 0;
  int max_depth_ = 0;
  uint32_t seed_ = 0xBABABEBEu;
  uint64_t batch_ = 1ull << 27;  // 134M paths (~19 GB of path state): per-bounce tails amortised

  uint32_t rank_ = 0, nranks_ = 1, tile_ = 16;
  std::vector<uint32_t> part_pix_;
  DevBuf<uint32_t> d_part_pix_;
  // each screen half's pixels of this rank: one rank in tile order; several
  // ranks as partition entries (indices into part_pix_) in partition order
  DevBuf<uint32_t> d_half_pix_[2];
  DevBuf<uint32_t> d_frame_pix_;                   // one rank: the frame's pixels, tile order
  uint32_t half_npix_[2] = {0, 0};
  uint64_t next_path_ = 0;

  DevBuf<float4> d_acc_;
  DevBuf<uint32_t> d_cnt_;
  DevBuf<uint8_t> d_rgba_;

  DevBuf<unsigned long long> d_work_;     // [kWorkCopies][kWorkWords] extend visits/tests/node bytes, shadow visits/tests/node bytes, ...
  PinBuf<uint32_t> h_word_;        // pinned scratch of the round planning (a round's path count)

  bool counting_ = false;
  bool profiling_ = false;
  Stats stats_;
  KernelTimes times_;
  struct PendingTiming {
    hipEvent_t a, b;
    int slot;
  };
  bool next_event(hipEvent_t* e, std::string& err);
  bool resolve_timings(std::string& err);
  std::vector<hipEvent_t> ev_pool_;
  size_t ev_used_ = 0;
  std::vector<PendingTiming> pending_;
};

}  // namespace wpt
