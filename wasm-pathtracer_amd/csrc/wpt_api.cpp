// wpt_api.cpp — the C ABI (include/wpt.h), mirroring src/wasm_interface.rs.
//
// The reference keeps one global session (`static mut CONFIG`,
// wasm_interface.rs:62) holding meshes, textures, the render target, the
// scene, the camera and two RenderInstances (left/right viewport halves).
// Here the session holds the same host-side state plus one wpt::Renderer
// that owns the GPU side; every reference `panic!` becomes a WPT_ERR_* code.
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/wpt.h"
#include "wpt_bvh_gpu.h"
#include "wpt_comm.h"
#include "wpt_obj.h"
#include "wpt_partition.h"
#include "wpt_render.h"
#include "wpt_seqsum.h"

using namespace wpt;

namespace {

#include "wpt_denoise.h"    // the host part: the restatement wpt_denoise_host runs
#include "wpt_reproject.h"  // likewise wpt_reproject_host's
#include "wpt_guided.h"     // and wpt_sample_map_host's
#include "wpt_upsample.h"   // and wpt_upsample_host's
#include "wpt_rays.h"       // the validity rule of a query ray
#include "wpt_points.h"     // point_ray: the ray of a point query's sample
#include "wpt_sh.h"         // sh_basis: the weights of an SH query's samples

struct Session {
  std::map<uint32_t, std::vector<float>> preload;   // Mesh::Preload (mesh.rs:8-13)
  std::map<uint32_t, std::vector<float>> meshes;    // Mesh::Triangled, as raw vertex triples
  std::map<uint32_t, std::vector<uint8_t>> textures;
  uint32_t scene_id = 0;
  HostScene scene;
  Renderer renderer;
  uint32_t width = 0, height = 0;
  float cam[5] = {0, 0, 0, 0, 0};
  // the reference's initial settings (wasm_interface.rs:90-94): left half
  // NormalNEE with random sampling, right half PNEE with adaptive sampling
  int left_type = WPT_NORMAL_NEE, right_type = WPT_PNEE, light_debug = 0;
  bool left_adaptive = false, right_adaptive = true;
  int max_depth = 0;
  uint32_t seed = 0xBABABEBEu;
  std::vector<uint8_t> rgba;       // RenderTarget.result (render_target.rs:10)
  std::vector<uint8_t> sampling;   // host copy of the SimpleRenderTarget (sampling visualisation)
  // multi-GPU (wpt_set_comm): the RCCL communicator, the packed partition of
  // this rank and the gathered partitions of all ranks (rank-major)
  Comm* comm = nullptr;
  DevBuf<float4> comm_send;  // comm_send.cap() float4: the slot of every rank
  DevBuf<float4> comm_recv;
  // or a caller's transport (wpt_set_transport) over caller-owned buffers
  wpt_transport_fn xfer = nullptr;
  void* xfer_user = nullptr;
  float4* xfer_send = nullptr;
  float4* xfer_recv = nullptr;
  uint64_t xfer_slot = 0;
  BvhGpu bvh_gpu;  // the GPU BVH2 build (wpt_bvh_gpu.h) for large scenes
  // wpt_probe_read's snapshot between its size query and its fill call
  std::vector<uint32_t> probe_meta;
  std::vector<uint4> probe_rec;
  double probe_tpu = 0.0;
  bool probe_taken = false;
  ~Session() { drop_comm(); }
  void drop_comm() {
    if (comm || xfer) renderer.set_exchange(nullptr, nullptr, nullptr, nullptr, 0);
    xfer = nullptr;
    xfer_user = nullptr;
    xfer_send = xfer_recv = nullptr;
    xfer_slot = 0;
    comm_destroy(comm);
    comm = nullptr;
    comm_send.reset();
    comm_recv.reset();
  }
};

Session* g_session = nullptr;
bool size_comm(Session& s);  // communicator buffers for the current partition (below)
int g_device = 0;
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// The mesh slot a scene displays (scenes.rs:16 MESH_BUNNY_HIGH = 1; the
// reference's notify_mesh_loaded maps scene 1/2/3 to mesh 0/1/2, :317-321).
int mesh_for_scene(uint32_t scene_id) {
  if (scene_id == 1) return 0;
  if (scene_id == 2) return 1;
  if (scene_id == 3) return 2;
  return -1;
}

// Where a scene's BVH2 is built (WPT_OPT_BVH_BUILD): 1 = host, 2 = GPU,
// 0 = the GPU for scenes of at least kGpuBvhShapes finite shapes (the same
// tree either way).
constexpr size_t kGpuBvhShapes = 65536;
int g_bvh_build = 0;
Bvh2Builder* scene_builder(BvhGpu& gpu) {
  if (g_bvh_build == 1) return nullptr;
  gpu.min_shapes = g_bvh_build == 2 ? 0 : kGpuBvhShapes;
  return &gpu;
}
// Options set with no session: the defaults of every later wpt_init.
std::map<int, int64_t> g_default_opts;

int rebuild_scene(Session& s, uint32_t scene_id) {
  std::string err;
  HostScene sc;
  // the BVH4 only feeds the fast-path traversal (WPT_OPT_TRAVERSAL(_SH))
  sc.want_bvh4 = s.renderer.wants_bvh4();
  static const std::vector<float> empty;
  int mid = mesh_for_scene(scene_id);
  const std::vector<float>* mesh = &empty;
  if (mid >= 0) {
    auto it = s.meshes.find((uint32_t)mid);
    if (it != s.meshes.end()) mesh = &it->second;
  }
  if (!build_scene((int)scene_id, *mesh, sc, err, scene_builder(s.bvh_gpu))) {
    if (err.rfind("HIP error", 0) == 0 || err.rfind("GPU BVH", 0) == 0) return fail(WPT_ERR_DEVICE, err);
    return fail(scene_id == 0 ? WPT_ERR_UNSUPPORTED : WPT_ERR_INVALID_SCENE, err);
  }
  if (!s.renderer.upload_scene(sc, err)) return fail(WPT_ERR_DEVICE, err);
  s.scene = std::move(sc);
  s.scene_id = scene_id;
  return WPT_OK;
}

int reset_session(Session& s) {  // wasm_interface.rs:137-150
  std::string err;
  if (!s.renderer.reset(err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

bool valid_type(uint32_t t) { return t <= 2u; }

}  // namespace

extern "C" {

const char* wpt_last_error(void) { return g_err.c_str(); }

int wpt_set_device(int device) {
  if (g_session) return fail(WPT_ERR_ALREADY_INIT, "device must be chosen before init");
  if (device < 0) return fail(WPT_ERR_INVALID_ARG, "bad device");
  g_device = device;
  return WPT_OK;
}

int wpt_init(uint32_t width, uint32_t height, uint32_t scene_id, float cam_x, float cam_y, float cam_z,
             float cam_rot_x, float cam_rot_y) {
  if (g_session) return fail(WPT_ERR_ALREADY_INIT, "Cannot init again");
  if (width == 0 || height == 0) return fail(WPT_ERR_INVALID_ARG, "empty viewport");
  std::unique_ptr<Session> s(new Session());
  std::string err;
  if (!s->renderer.set_device(g_device, err)) return fail(WPT_ERR_DEVICE, err);
  s->width = width;
  s->height = height;
  float cam[5] = {cam_x, cam_y, cam_z, cam_rot_x, cam_rot_y};
  memcpy(s->cam, cam, sizeof cam);
  s->renderer.set_camera(cam);
  s->renderer.set_types(s->left_type, s->right_type, s->light_debug);
  s->renderer.set_adaptive(s->left_adaptive, s->right_adaptive);
  s->renderer.set_options(s->max_depth, s->seed, 0);
  for (const auto& o : g_default_opts)
    if (!s->renderer.set_option(o.first, o.second, err)) return fail(WPT_ERR_INVALID_ARG, err);
  if (!s->renderer.set_viewport(width, height, err)) return fail(WPT_ERR_DEVICE, err);
  int rc = rebuild_scene(*s, scene_id);
  if (rc != WPT_OK) return rc;
  s->rgba.assign((size_t)width * height * 4, 0);
  s->sampling.assign((size_t)width * height * 4, 0);
  // both strategies' constructors paint their halves blue (sampling_strategy.rs:42-51, :205-213)
  if (!s->renderer.fill_sampling_blue(err)) return fail(WPT_ERR_DEVICE, err);
  g_session = s.release();
  return WPT_OK;
}

const uint8_t* wpt_results(uint32_t is_show_sampling) {
  if (!g_session) { fail(WPT_ERR_NOT_INIT, "init not called"); return nullptr; }
  Session& s = *g_session;
  std::string err;
  if (is_show_sampling == 1) {
    if (!s.renderer.sampling_rgba(s.sampling.data(), err)) { fail(WPT_ERR_DEVICE, err); return nullptr; }
    return s.sampling.data();
  }
  if (!s.renderer.results_rgba(s.rgba.data(), err)) { fail(WPT_ERR_DEVICE, err); return nullptr; }
  return s.rgba.data();
}

int wpt_update_scene(uint32_t scene_id) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  int rc = rebuild_scene(*g_session, scene_id);
  if (rc != WPT_OK) return rc;
  return reset_session(*g_session);
}

int wpt_update_settings(uint32_t left_type, uint32_t right_type, uint32_t is_left_adaptive, uint32_t is_right_adaptive,
                        uint32_t is_light_debug) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!valid_type(left_type) || !valid_type(right_type)) return fail(WPT_ERR_INVALID_ARG, "Invalid RenderType magic number");
  Session& s = *g_session;
  s.left_type = (int)left_type;
  s.right_type = (int)right_type;
  s.light_debug = is_light_debug == 1 ? 1 : 0;
  s.left_adaptive = is_left_adaptive == 1;
  s.right_adaptive = is_right_adaptive == 1;
  s.renderer.set_types(s.left_type, s.right_type, s.light_debug);
  s.renderer.set_adaptive(s.left_adaptive, s.right_adaptive);
  // new strategies, then target and sampling view cleared and the instances
  // reset (wasm_interface.rs:185-201): random halves black, adaptive blue
  return reset_session(s);
}

int wpt_update_viewport(uint32_t width, uint32_t height) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (width == 0 || height == 0) return fail(WPT_ERR_INVALID_ARG, "empty viewport");
  Session& s = *g_session;
  std::string err;
  if (!s.renderer.set_viewport(width, height, err)) return fail(WPT_ERR_DEVICE, err);
  s.width = width;
  s.height = height;
  s.rgba.assign((size_t)width * height * 4, 0);
  s.sampling.assign((size_t)width * height * 4, 0);
  if (s.comm && !size_comm(s)) return fail(WPT_ERR_DEVICE, "hipMalloc failed (communicator buffers)");
  return WPT_OK;  // set_viewport reset the session (wasm_interface.rs:219-232)
}

int wpt_update_camera(float cam_x, float cam_y, float cam_z, float cam_rot_x, float cam_rot_y) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  Session& s = *g_session;
  float cam[5] = {cam_x, cam_y, cam_z, cam_rot_x, cam_rot_y};
  memcpy(s.cam, cam, sizeof cam);
  s.renderer.set_camera(cam);
  return reset_session(s);
}

int wpt_allocate_mesh(uint32_t id, uint32_t num_vertices) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  g_session->preload[id].assign((size_t)num_vertices * 3, 0.0f);
  return WPT_OK;
}

int wpt_parse_obj(const char* text, size_t len, const float* scale, float* out, uint64_t capacity,
                  uint64_t* num_vertices) {
  if (!text && len) return fail(WPT_ERR_INVALID_ARG, "null text");
  std::vector<float> v;
  std::string err;
  if (!parse_obj(text, len, v, err)) return fail(WPT_ERR_INVALID_ARG, err);
  if (scale) scale_vertices(v, scale);
  if (num_vertices) *num_vertices = v.size() / 3;
  if (out) {
    if (capacity < v.size() / 3) return fail(WPT_ERR_INVALID_ARG, "output too small");
    std::memcpy(out, v.data(), v.size() * sizeof(float));
  }
  return WPT_OK;
}

int wpt_load_obj(uint32_t id, const char* text, size_t len, const float* scale, uint64_t* num_vertices) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!text && len) return fail(WPT_ERR_INVALID_ARG, "null text");
  std::vector<float> v;
  std::string err;
  if (!parse_obj(text, len, v, err)) return fail(WPT_ERR_INVALID_ARG, err);
  if (scale) scale_vertices(v, scale);
  if (num_vertices) *num_vertices = v.size() / 3;
  g_session->preload[id] = std::move(v);  // as allocate_mesh + mesh_vertices
  return WPT_OK;
}

float* wpt_mesh_vertices(uint32_t id) {
  if (!g_session) { fail(WPT_ERR_NOT_INIT, "init not called"); return nullptr; }
  auto it = g_session->preload.find(id);
  if (it == g_session->preload.end()) { fail(WPT_ERR_NO_MESH, "Mesh not allocated"); return nullptr; }
  return it->second.data();
}

int wpt_notify_mesh_loaded(uint32_t id) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  Session& s = *g_session;
  auto it = s.preload.find(id);
  if (it != s.preload.end()) {
    // wasm_interface.rs:300-311: num_triangles = len/3 (vertices), the
    // ×0.5 / +z5 transform is applied when the scene is assembled.
    std::vector<float> v = std::move(it->second);
    v.resize((v.size() / 9) * 9);
    s.meshes[id] = std::move(v);
    s.preload.erase(it);
  }
  if (mesh_for_scene(s.scene_id) == (int)id) {
    int rc = wpt_update_scene(s.scene_id);
    return rc == WPT_OK ? 1 : rc;
  }
  return 0;
}

uint8_t* wpt_allocate_texture(uint32_t id, uint32_t width, uint32_t height) {
  if (!g_session) { fail(WPT_ERR_NOT_INIT, "init not called"); return nullptr; }
  auto& t = g_session->textures[id];
  t.assign((size_t)width * height * 3, 0);
  return t.data();
}

int wpt_notify_texture_loaded(uint32_t) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  return 0;  // textures are never sampled (material.rs:53-60)
}

int wpt_compute(size_t num_samples) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  // a map's samples start at each pixel's count; the sequences below take their
  // sample indices from round and position counters and would repeat them
  if (g_session->renderer.map_mode())
    return fail(WPT_ERR_INVALID_ARG,
                "compute: the session is in map mode (wpt_compute_map traced a sample map) until the accumulation "
                "is reset");
  if (!g_session->renderer.compute((uint64_t)num_samples, err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_set_render_options(int32_t max_depth, uint32_t frame_seed, uint64_t batch_paths) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (max_depth < 0) return fail(WPT_ERR_INVALID_ARG, "max_depth < 0");
  Session& s = *g_session;
  s.max_depth = max_depth;
  s.seed = frame_seed;
  s.renderer.set_options(max_depth, frame_seed, batch_paths);
  return reset_session(s);
}

int wpt_set_partition(uint32_t rank, uint32_t nranks, uint32_t tile) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  if (!g_session->renderer.set_partition(rank, nranks, tile, err)) return fail(WPT_ERR_INVALID_ARG, err);
  return WPT_OK;
}

int64_t wpt_partition_pixels(uint32_t* out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  int64_t n = g_session->renderer.part_pixels();
  if (out) {
    const std::vector<uint32_t>& l = g_session->renderer.part_list();
    memcpy(out, l.data(), sizeof(uint32_t) * l.size());
  }
  return n;
}

int64_t wpt_tile_partition(uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks, uint32_t tile,
                           uint32_t* out) {
  if (nranks == 0 || rank >= nranks || tile == 0) return fail(WPT_ERR_INVALID_ARG, "bad partition");
  std::vector<uint32_t> l;
  wpt::tile_partition(width, height, rank, nranks, tile, l);
  if (out) memcpy(out, l.data(), sizeof(uint32_t) * l.size());
  return (int64_t)l.size();
}

int64_t wpt_photon_tree(uint32_t* child, float* cum, uint64_t* shot_stored) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::vector<uint32_t> c;
  std::vector<float> f;
  uint64_t shot = 0, stored = 0;
  std::string err;
  if (!g_session->renderer.photon_tree(c, f, shot, stored, err)) return fail(WPT_ERR_DEVICE, err);
  if (child) memcpy(child, c.data(), sizeof(uint32_t) * c.size());
  if (cum) memcpy(cum, f.data(), sizeof(float) * f.size());
  if (shot_stored) { shot_stored[0] = shot; shot_stored[1] = stored; }
  return (int64_t)c.size();
}

int64_t wpt_photon_build(uint32_t num_lights, uint64_t n, const uint32_t* light, const float* loc3,
                         const float* intensity, uint32_t* child, float* cum, uint32_t* corners) {
  if (n && (!light || !loc3 || !intensity)) return fail(WPT_ERR_INVALID_ARG, "null argument");
  for (uint64_t i = 0; i < n; i++)
    if (light[i] >= num_lights) return fail(WPT_ERR_INVALID_ARG, "photon light id out of range");
  wpt::PhotonTree tree(num_lights);
  for (uint64_t i = 0; i < n; i++) tree.insert(light[i], mk(loc3[3 * i], loc3[3 * i + 1], loc3[3 * i + 2]), intensity[i]);
  std::vector<uint32_t> c, t;
  std::vector<float> f;
  tree.freeze(c, f);
  if (child) memcpy(child, c.data(), sizeof(uint32_t) * c.size());
  if (cum) memcpy(cum, f.data(), sizeof(float) * f.size());
  if (corners) {
    wpt::oct_corner_table(c, t);
    memcpy(corners, t.data(), sizeof(uint32_t) * t.size());
  }
  return (int64_t)c.size();
}

int wpt_install_photons(uint64_t n, const uint32_t* light, const float* loc3, const float* intensity) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (n && (!light || !loc3 || !intensity)) return fail(WPT_ERR_INVALID_ARG, "null argument");
  std::string err;
  const int rc = g_session->renderer.install_photons(n, light, loc3, intensity, err);
  if (rc <= 0) return fail(rc < 0 ? WPT_ERR_INVALID_ARG : WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_photon_sample(size_t n, const float* points3, const uint32_t* states, int32_t view, int32_t table,
                      uint32_t* light, float* pdf, uint32_t* states_out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (n && (!points3 || !states || !light || !pdf || !states_out)) return fail(WPT_ERR_INVALID_ARG, "null argument");
  if (view < 0 || view > 2) return fail(WPT_ERR_INVALID_ARG, "photon_sample: view 0, 1 or 2");
  std::string err;
  const int rc = g_session->renderer.photon_sample(n, points3, states, view, table != 0, light, pdf, states_out, err);
  if (rc <= 0) return fail(rc < 0 ? WPT_ERR_INVALID_ARG : WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_read_radiance(float* acc3, uint32_t* cnt) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!acc3) return fail(WPT_ERR_INVALID_ARG, "null buffer");
  std::string err;
  if (!g_session->renderer.read_radiance(acc3, cnt, err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_copy_partition(void* device_dst) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  if (!g_session->renderer.copy_partition((float*)device_dst, err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_set_exchange(wpt_exchange_fn fn, void* user, void* local_dev, void* gathered_dev, uint64_t slot) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (fn && (!local_dev || !gathered_dev)) return fail(WPT_ERR_INVALID_ARG, "null exchange buffer");
  if (fn && slot < g_session->renderer.exchange_slot()) return fail(WPT_ERR_INVALID_ARG, "exchange slot too small");
  g_session->renderer.set_exchange(fn, user, local_dev, gathered_dev, slot);
  return WPT_OK;
}

int64_t wpt_exchange_slot(void) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  return (int64_t)g_session->renderer.exchange_slot();
}

// ---- RCCL communicator ------------------------------------------
namespace {
// wpt_set_exchange callback of a communicator session: the library has
// packed this rank's partition into comm_send; all-gather every rank's.
int comm_exchange(void* user) {
  Session& s = *(Session*)user;
  std::string err;
  if (!comm_allgather(s.comm, s.comm_send, s.comm_recv, s.comm_send.cap(), s.renderer.stream(), err)) {
    g_err = err;
    return 1;
  }
  return 0;
}
// The communicator's send / receive buffers sized for this rank's partition
// and the largest one (they grow with the viewport: wpt_update_viewport keeps
// the partition), registered as the adaptive rounds' frame exchange.
bool size_comm(Session& s) {
  uint64_t slot = std::max<uint64_t>(s.renderer.exchange_slot(), s.renderer.part_pixels());
  if (slot == 0) slot = 1;
  if (slot > s.comm_send.cap()) {
    s.comm_send.reset();
    s.comm_recv.reset();
    if (s.comm_send.alloc(slot) != hipSuccess || s.comm_recv.alloc(slot * comm_size(s.comm)) != hipSuccess) {
      s.comm_send.reset();  // (its capacity is the slot both buffers hold)
      return false;
    }
  }
  // adaptive rounds exchange the frame over the communicator
  s.renderer.set_exchange(comm_exchange, &s, s.comm_send, s.comm_recv, s.comm_send.cap());
  return true;
}
}  // namespace

int wpt_comm_unique_id(void* out) {
  if (!out) return fail(WPT_ERR_INVALID_ARG, "null id buffer");
  std::string err;
  if (!comm_unique_id(out, err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_set_comm(uint32_t rank, uint32_t nranks, uint32_t tile, const void* unique_id) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!unique_id || nranks == 0 || rank >= nranks || tile == 0) return fail(WPT_ERR_INVALID_ARG, "bad communicator");
  Session& s = *g_session;
  s.drop_comm();
  std::string err;
  if (!s.renderer.set_partition(rank, nranks, tile, err)) return fail(WPT_ERR_INVALID_ARG, err);
  if (hipSetDevice(g_device) != hipSuccess) return fail(WPT_ERR_DEVICE, "hipSetDevice failed");
  s.comm = comm_create(rank, nranks, unique_id, err);
  if (!s.comm) return fail(WPT_ERR_DEVICE, err);
  if (!size_comm(s)) {
    s.drop_comm();
    return fail(WPT_ERR_DEVICE, "hipMalloc failed (communicator buffers)");
  }
  return WPT_OK;
}

int wpt_gather_frame(uint32_t root) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  Session& s = *g_session;
  if (s.xfer) {
    // the caller's transport: pack, let it move the rank-major buffers, unpack
    std::string err;
    const Renderer& r = s.renderer;
    if (root >= r.nranks()) return fail(WPT_ERR_INVALID_ARG, "bad root");
    if (s.xfer_slot < r.exchange_slot()) return fail(WPT_ERR_INVALID_ARG, "transport slot smaller than the largest partition");
    if (!s.renderer.copy_partition((float*)s.xfer_send, err)) return fail(WPT_ERR_DEVICE, err);
    if (s.xfer(s.xfer_user, WPT_XFER_GATHER, root) != 0) return fail(WPT_ERR_DEVICE, "transport gather failed");
    if (r.rank() == root && !s.renderer.unpack_ranks(s.xfer_recv, s.xfer_slot, err)) return fail(WPT_ERR_DEVICE, err);
    return WPT_OK;
  }
  if (!s.comm) return fail(WPT_ERR_INVALID_ARG, "no communicator (wpt_set_comm / wpt_set_transport)");
  if (root >= comm_size(s.comm)) return fail(WPT_ERR_INVALID_ARG, "bad root");
  if (!size_comm(s)) return fail(WPT_ERR_DEVICE, "hipMalloc failed (communicator buffers)");
  std::string err;
  if (!s.renderer.copy_partition((float*)s.comm_send.get(), err)) return fail(WPT_ERR_DEVICE, err);
  if (!comm_gather(s.comm, s.comm_send, s.comm_recv, s.comm_send.cap(), root, s.renderer.stream(), err))
    return fail(WPT_ERR_DEVICE, err);
  if (comm_rank(s.comm) == root && !s.renderer.unpack_ranks(s.comm_recv, s.comm_send.cap(), err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

namespace {
// adaptive rounds' frame exchange through the caller's transport
int xfer_exchange(void* user) {
  Session& s = *(Session*)user;
  return s.xfer(s.xfer_user, WPT_XFER_ALLGATHER, 0);
}
}  // namespace

int wpt_set_transport(wpt_transport_fn fn, void* user, void* send_dev, void* recv_dev, uint64_t slot) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  Session& s = *g_session;
  if (!fn) {
    // unregister the transport only (an RCCL communicator, if any, stays)
    if (s.xfer) {
      s.renderer.set_exchange(nullptr, nullptr, nullptr, nullptr, 0);
      s.xfer = nullptr;
      s.xfer_user = nullptr;
      s.xfer_send = s.xfer_recv = nullptr;
      s.xfer_slot = 0;
    }
    return WPT_OK;
  }
  // validate first: a rejected registration leaves the session as it was
  if (!send_dev || !recv_dev) return fail(WPT_ERR_INVALID_ARG, "null transport buffer");
  if (slot < s.renderer.exchange_slot() || slot < s.renderer.part_pixels())
    return fail(WPT_ERR_INVALID_ARG, "transport slot smaller than the largest partition");
  s.drop_comm();  // a transport replaces the RCCL communicator (include/wpt.h)
  s.xfer = fn;
  s.xfer_user = user;
  s.xfer_send = (float4*)send_dev;
  s.xfer_recv = (float4*)recv_dev;
  s.xfer_slot = slot;
  s.renderer.set_exchange(xfer_exchange, &s, send_dev, recv_dev, slot);
  return WPT_OK;
}

int64_t wpt_gather_plan(uint32_t rank, uint32_t nranks, uint32_t root, uint64_t slot, uint64_t* out) {
  if (nranks == 0 || rank >= nranks || root >= nranks) return fail(WPT_ERR_INVALID_ARG, "bad rank");
  std::vector<XferOp> ops;
  gather_plan(rank, nranks, root, slot, ops);
  if (out)
    for (size_t i = 0; i < ops.size(); i++) {
      out[4 * i] = ops[i].peer;
      out[4 * i + 1] = ops[i].offset;
      out[4 * i + 2] = ops[i].count;
      out[4 * i + 3] = ops[i].recv ? 1u : 0u;
    }
  return (int64_t)ops.size();
}

float wpt_seq_sum(const float* v, uint64_t n) { return wpt::seq_sum_f32(v, (size_t)n); }

float wpt_seq_sum_chunks(const float* v, uint64_t n) {
  std::vector<wpt::ChunkEff> eff(2 * ((size_t)n / wpt::kSumChunk + 1));
  wpt::seq_sum_effects(v, (size_t)n, eff.data());
  return wpt::seq_sum_walk(v, (size_t)n, eff.data());
}

int wpt_seq_sum_device(const float* v, uint64_t n, float* out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!out || (n && !v)) return fail(WPT_ERR_INVALID_ARG, "null pointer");
  std::string err;
  if (!g_session->renderer.seq_sum_device(v, n, *out, err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_adaptive_error(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, uint32_t half, float* mse_out,
                       float* stats3_out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!acc3 || !cnt || !mse_out || !stats3_out) return fail(WPT_ERR_INVALID_ARG, "null pointer");
  if (half > 1) return fail(WPT_ERR_INVALID_ARG, "adaptive_error: half 0 or 1");
  if ((uint64_t)W * H == 0 || (uint64_t)W * H >= (1ull << 32)) return fail(WPT_ERR_INVALID_ARG, "bad frame size");
  std::string err;
  if (!g_session->renderer.adaptive_error(W, H, acc3, cnt, (int)half, mse_out, stats3_out, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_adaptive_plan(uint32_t W, uint32_t H, uint32_t half, int32_t first, int32_t adaptive, const float* mse_in,
                      const float* stats3_in, const uint32_t* cnt_in, uint32_t* count_out, uint32_t* offset_out,
                      uint32_t* base_out, uint8_t* samp) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!mse_in || !stats3_in || !cnt_in || !count_out || !offset_out || !base_out || !samp)
    return fail(WPT_ERR_INVALID_ARG, "null pointer");
  if (half > 1) return fail(WPT_ERR_INVALID_ARG, "adaptive_plan: half 0 or 1");
  if ((uint64_t)W * H == 0 || (uint64_t)W * H >= (1ull << 32)) return fail(WPT_ERR_INVALID_ARG, "bad frame size");
  std::string err;
  if (!g_session->renderer.adaptive_plan(W, H, (int)half, first != 0, adaptive != 0, mse_in, stats3_in, cnt_in,
                                         count_out, offset_out, base_out, samp, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_comm_destroy(void) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  g_session->drop_comm();
  return WPT_OK;
}

int wpt_stats(uint64_t* out, size_t n) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  if (!g_session->renderer.flush_counts(err)) return fail(WPT_ERR_DEVICE, err);
  const Stats& st = g_session->renderer.stats();
  uint64_t v[44] = {st.paths,          st.rays,           st.shadow_rays,    st.node_visits,  st.prim_tests,
                    st.bounces,        st.ext_visits,     st.ext_tests,      st.ext_node_bytes, st.sh_visits,
                    st.sh_tests,       st.sh_node_bytes,  st.fallback_ext,   st.fallback_sh,  st.ext_lane_iters,
                    st.ext_live_iters, st.sh_lane_iters,  st.sh_live_iters,  st.photon_rays,  st.photons,
                    st.sum_chunks,     st.sum_resummed,   st.sum_fetched,    st.stock_consumed, st.fill_paths,
                    st.trace_bytes,    st.finish_paths,   st.finish_max_bounces, st.max_ray_visits,
                    st.ex_body_lanes,  st.ex_bodies,      st.lf_body_lanes,  st.lf_bodies,    st.stock_traced,
                    st.stock_deficit,  st.stock_waits,    st.plan_us,        st.stock_us,
                    st.stock_rays,     st.stock_rays_used, st.presolved_rays,
                    st.dropped_rays,   st.shadow_presolved_rays, st.gen_shaded_rays};
  for (size_t i = 0; i < n && i < 44; i++) out[i] = v[i];
  return WPT_OK;
}

int wpt_kernel_times(double* out, size_t n) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  const KernelTimes& t = g_session->renderer.times();
  double v[28] = {t.generate, (double)t.n_generate, t.extend, (double)t.n_extend, t.shade, (double)t.n_shade,
                  t.shadow, (double)t.n_shadow, t.accumulate, (double)t.n_accumulate, t.trace, (double)t.n_trace};
  for (int k = 0; k < 6; k++) {
    v[12 + 2 * k] = t.busy[k];
    v[13 + 2 * k] = (double)t.logical[k];
  }
  v[24] = t.retrace;
  v[25] = (double)t.n_retrace;
  v[26] = t.busy[6];
  v[27] = (double)t.logical[6];
  for (size_t i = 0; i < n && i < 28; i++) out[i] = v[i];
  return WPT_OK;
}

int wpt_set_counting(int on) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  g_session->renderer.set_counting(on != 0);
  return WPT_OK;
}

int wpt_scene_build_info(double* out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!out) return fail(WPT_ERR_INVALID_ARG, "null argument");
  out[0] = g_session->scene.bvh_ms;
  out[1] = g_session->scene.bvh_on_gpu ? 1.0 : 0.0;
  return WPT_OK;
}

int wpt_set_lanes(int32_t n) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (!g_session->renderer.set_lanes(n)) return fail(WPT_ERR_INVALID_ARG, "lanes out of range");
  return WPT_OK;
}

int wpt_set_option(int32_t option, int64_t value) {
  if (option == WPT_OPT_BVH_BUILD) {
    if (value < 0 || value > 2) return fail(WPT_ERR_INVALID_ARG, "option value out of range");
    g_bvh_build = (int)value;  // the next scene build
    return WPT_OK;
  }
  std::string err;
  if (!g_session) {
    if (option == WPT_OPT_DEFAULTS) {  // back to the built-in defaults
      g_default_opts.clear();
      g_bvh_build = 0;
      return WPT_OK;
    }
    // validated against a scratch renderer's ranges, applied at wpt_init
    if (option == WPT_OPT_LANES && (value < 1 || value > kMaxLanes)) return fail(WPT_ERR_INVALID_ARG, "lanes out of range");
    if (option != WPT_OPT_LANES && option != WPT_OPT_GRID_PCT) {
      Renderer probe;
      if (!probe.set_option(option, value, err)) return fail(WPT_ERR_INVALID_ARG, err);
    } else if (option == WPT_OPT_GRID_PCT && (value < 1 || value > 100)) {
      return fail(WPT_ERR_INVALID_ARG, "option value out of range");
    }
    g_default_opts[option] = value;
    return WPT_OK;
  }
  Session& s = *g_session;
  int64_t prev = 0;
  const bool had = s.renderer.get_option(option, prev);
  if (!s.renderer.set_option(option, value, err)) return fail(WPT_ERR_INVALID_ARG, err);
  if (Renderer::scene_option(option)) {
    // the device scene carries the traversal's nodes: re-upload it; if that
    // fails, the option goes back to its previous value
    const int rc = rebuild_scene(s, s.scene_id);
    if (rc != WPT_OK) {
      const std::string keep = g_err;
      std::string e2;
      if (had) (void)s.renderer.set_option(option, prev, e2);
      g_err = keep;
      return rc;
    }
    return reset_session(s);
  }
  if (option == WPT_OPT_PIXEL_TILE && s.renderer.nranks() == 1) {
    // the tile order only shapes a one-rank partition (several ranks keep
    // their tiles: nothing to redo)
    if (!s.renderer.set_partition(s.renderer.rank(), s.renderer.nranks(), s.renderer.tile(), err))
      return fail(WPT_ERR_DEVICE, err);
  }
  return WPT_OK;
}

int64_t wpt_probe_read(uint32_t* meta, uint32_t* rec, uint64_t* rec_entries, double* ticks_per_us) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  Session& s = *g_session;
  std::string err;
  if (!meta || !rec) {
    // the size query takes the snapshot (the session keeps it); the fill
    // call below copies it out (no function-static buffers)
    if (!s.renderer.probe_read(s.probe_meta, s.probe_rec, s.probe_tpu, err)) return fail(WPT_ERR_DEVICE, err);
    s.probe_taken = true;
    if (rec_entries) *rec_entries = s.probe_rec.size();
    if (ticks_per_us) *ticks_per_us = s.probe_tpu;
    return (int64_t)(s.probe_meta.size() / 5);
  }
  // fill: *rec_entries holds rec's capacity in entries; meta must hold 5 x
  // the launches the size query returned
  if (!s.probe_taken) return fail(WPT_ERR_INVALID_ARG, "probe: call with meta = rec = NULL first (size query)");
  if (!rec_entries || *rec_entries < s.probe_rec.size())
    return fail(WPT_ERR_INVALID_ARG, "probe: rec smaller than the size query's entries");
  std::memcpy(meta, s.probe_meta.data(), s.probe_meta.size() * sizeof(uint32_t));
  std::memcpy(rec, s.probe_rec.data(), s.probe_rec.size() * sizeof(uint4));
  *rec_entries = s.probe_rec.size();
  if (ticks_per_us) *ticks_per_us = s.probe_tpu;
  const int64_t n = (int64_t)(s.probe_meta.size() / 5);
  s.probe_meta.clear();
  s.probe_rec.clear();
  s.probe_taken = false;
  return n;
}

int wpt_get_option(int32_t option, int64_t* value) {
  if (!value) return fail(WPT_ERR_INVALID_ARG, "null argument");
  if (option == WPT_OPT_BVH_BUILD) { *value = g_bvh_build; return WPT_OK; }
  if (!g_session) {
    auto it = g_default_opts.find(option);
    if (it != g_default_opts.end()) { *value = it->second; return WPT_OK; }
    Renderer probe;
    if (!probe.get_option(option, *value)) return fail(WPT_ERR_INVALID_ARG, "unknown option");
    return WPT_OK;
  }
  if (!g_session->renderer.get_option(option, *value)) return fail(WPT_ERR_INVALID_ARG, "unknown option");
  return WPT_OK;
}

int wpt_set_profiling(int on) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  g_session->renderer.set_profiling(on != 0);
  return WPT_OK;
}

int wpt_clear_stats(void) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  g_session->renderer.clear_stats();
  return WPT_OK;
}

int wpt_sync(void) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  if (!g_session->renderer.sync(err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_bvh_depth(void) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  return (int)g_session->renderer.bvh_depth();
}

int wpt_trace_rays(size_t n, const float* rays, float* t_out, int32_t* id_out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  if (!g_session->renderer.trace_rays(n, rays, t_out, id_out, err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_first_hit(uint32_t sample, float* dir3, float* t, int32_t* id, uint32_t* visits, float* normal3,
                  float* albedo3, uint8_t* kind) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  if (!g_session->renderer.first_hit(sample, dir3, t, id, visits, normal3, albedo3, kind, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

namespace {
// scale^2 * W * H >= 2^32: a fine pixel's index would not fit 32 bits
bool scaled_too_large(uint32_t W, uint32_t H, uint32_t scale) {
  const uint64_t np = (uint64_t)W * H;
  return np >= (1ull << 32) || np * scale * scale >= (1ull << 32);
}
}  // namespace

int wpt_first_hit_scaled(uint32_t scale, uint32_t sample, float* dir3, float* t, int32_t* id, uint32_t* visits,
                         float* normal3, float* albedo3, uint8_t* kind) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (scale == 0 || scale > kUpMaxScale) return fail(WPT_ERR_INVALID_ARG, "first_hit_scaled: scale 1..4");
  if (scaled_too_large(g_session->renderer.width(), g_session->renderer.height(), scale))
    return fail(WPT_ERR_INVALID_ARG, "first_hit_scaled: the scaled viewport has 2^32 pixels or more");
  std::string err;
  if (!g_session->renderer.first_hit_scaled(scale, sample, dir3, t, id, visits, normal3, albedo3, kind, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

// gen_path's ray on the host: the same primary_dir (wpt_math.h) over the
// constants Renderer::gen_params makes.
int wpt_primary_rays(uint32_t width, uint32_t height, const float* cam5, uint32_t frame_seed, uint32_t sample,
                     float* rays6) {
  if (width == 0 || height == 0) return fail(WPT_ERR_INVALID_ARG, "empty viewport");
  if (!cam5 || !rays6) return fail(WPT_ERR_INVALID_ARG, "null argument");
  const View v = make_view(width, height, cam5[3], cam5[4]);
  for (uint32_t y = 0; y < height; y++)
    for (uint32_t x = 0; x < width; x++) {
      const uint32_t pixel = y * width + x;
      uint32_t s = path_seed(frame_seed, pixel, sample);
      const V3 d = primary_dir(x, y, s, v.w_inv, v.h_inv, v.ar, v.cx, v.sx, v.cy, v.sy);
      float* r = rays6 + 6 * (size_t)pixel;
      r[0] = cam5[0]; r[1] = cam5[1]; r[2] = cam5[2];
      r[3] = d.x; r[4] = d.y; r[5] = d.z;
    }
  return WPT_OK;
}

namespace {
// the argument rules wpt_denoise, wpt_denoise_planes and wpt_denoise_host share
const char* denoise_args(uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags) {
  if (iterations == 0 || iterations > kDnMaxIter) return "denoise: iterations 1..5";
  if (!dn_finite(sigma_c) || !(sigma_c > 0.0f) || !dn_finite(sigma_z) || !(sigma_z > 0.0f))
    return "denoise: sigmas must be finite and > 0";
  if (flags & ~(uint32_t)WPT_DENOISE_ALBEDO) return "denoise: unknown flag";
  return nullptr;
}
const char* denoise_plane_args(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, const float* t,
                               const float* normal3, const float* albedo3, const uint8_t* kind) {
  if (!acc3 || !cnt || !t || !normal3 || !albedo3 || !kind) return "null pointer";
  if ((uint64_t)W * H == 0 || (uint64_t)W * H >= (1ull << 32)) return "bad frame size";
  return nullptr;
}
}  // namespace

int wpt_denoise(uint32_t sample, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags, float* rgb3,
                uint8_t* valid, uint8_t* rgba) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = denoise_args(iterations, sigma_c, sigma_z, flags)) return fail(WPT_ERR_INVALID_ARG, e);
  std::string err;
  if (!g_session->renderer.denoise(sample, iterations, sigma_c, sigma_z, flags, rgb3, valid, rgba, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_denoise_planes(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, const float* t,
                       const float* normal3, const float* albedo3, const uint8_t* kind, uint32_t iterations,
                       float sigma_c, float sigma_z, uint32_t flags, float* rgb3, uint8_t* valid, uint8_t* rgba) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = denoise_args(iterations, sigma_c, sigma_z, flags)) return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = denoise_plane_args(W, H, acc3, cnt, t, normal3, albedo3, kind)) return fail(WPT_ERR_INVALID_ARG, e);
  std::string err;
  Renderer& r = g_session->renderer;
  Guides g;
  g.t = t; g.normal = normal3; g.albedo = albedo3; g.kind = kind;
  if (!r.post().denoise_planes(r.stream(), HostFrame{W, H, acc3, cnt}, g, DnParams{iterations, sigma_c, sigma_z, flags},
                               PostOut{rgb3, valid, rgba}, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_denoise_host(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, const float* t,
                     const float* normal3, const float* albedo3, const uint8_t* kind, uint32_t iterations,
                     float sigma_c, float sigma_z, uint32_t flags, float* rgb3, uint8_t* valid, uint8_t* rgba) {
  if (const char* e = denoise_args(iterations, sigma_c, sigma_z, flags)) return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = denoise_plane_args(W, H, acc3, cnt, t, normal3, albedo3, kind)) return fail(WPT_ERR_INVALID_ARG, e);
  denoise_host(W, H, acc3, cnt, t, normal3, albedo3, kind, iterations, sigma_c, sigma_z, flags, rgb3, valid, rgba);
  return WPT_OK;
}

namespace {
// the argument rules the reprojection entry points share; KEEP is the session call's alone
const char* reproject_args(float cos_min, float eps_z, uint32_t max_len, uint32_t flags, uint32_t known) {
  if (!dn_finite(cos_min) || !(cos_min >= -1.0f) || !(cos_min <= 1.0f)) return "reproject: cos_min must be in [-1, 1]";
  if (!dn_finite(eps_z) || !(eps_z >= 0.0f)) return "reproject: eps_z must be finite and >= 0";
  if (max_len == 0 || max_len > kRpMaxLen) return "reproject: max_len 1..2^24";
  if (flags & ~known) return "reproject: unknown flag";
  return nullptr;
}
const char* reproject_plane_args(uint32_t W, uint32_t H, std::initializer_list<const void*> in) {
  for (const void* p : in)
    if (!p) return "null pointer";
  if ((uint64_t)W * H == 0 || (uint64_t)W * H >= (1ull << 32)) return "bad frame size";
  return nullptr;
}
constexpr uint32_t kRpPlaneFlags = WPT_REPROJECT_NEAREST | WPT_REPROJECT_SAME_SHAPE;
}  // namespace

int wpt_reproject(uint32_t sample, float cos_min, float eps_z, uint32_t max_len, uint32_t flags, float* acc3,
                  uint32_t* cnt, uint32_t* len) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = reproject_args(cos_min, eps_z, max_len, flags, kRpPlaneFlags | WPT_REPROJECT_KEEP))
    return fail(WPT_ERR_INVALID_ARG, e);
  if (g_session->renderer.history_state() == 2)
    return fail(WPT_ERR_INVALID_ARG, "reproject: the history already holds this accumulation");
  std::string err;
  if (!g_session->renderer.reproject(sample, cos_min, eps_z, max_len, flags, acc3, cnt, len, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_history_drop(void) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  g_session->renderer.history_drop();
  return WPT_OK;
}

int wpt_denoise_merged(uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags, float* rgb3, uint8_t* valid,
                       uint8_t* rgba) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = denoise_args(iterations, sigma_c, sigma_z, flags)) return fail(WPT_ERR_INVALID_ARG, e);
  if (!g_session->renderer.has_merged())
    return fail(WPT_ERR_INVALID_ARG, "denoise_merged: no wpt_reproject since the viewport was set");
  std::string err;
  if (!g_session->renderer.denoise_merged(iterations, sigma_c, sigma_z, flags, rgb3, valid, rgba, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

namespace {
// the argument rules the upsampling entry points share; MERGED is the session call's alone
const char* upsample_args(uint32_t scale, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags,
                          uint32_t known) {
  if (scale < 2 || scale > kUpMaxScale) return "upsample: scale 2..4";
  if (iterations > kDnMaxIter) return "upsample: iterations 0..5";
  if (!dn_finite(sigma_c) || !(sigma_c > 0.0f) || !dn_finite(sigma_z) || !(sigma_z > 0.0f))
    return "upsample: sigmas must be finite and > 0";
  if (flags & ~known) return "upsample: unknown flag";
  return nullptr;
}
const char* upsample_plane_args(uint32_t W, uint32_t H, uint32_t scale, std::initializer_list<const void*> in) {
  for (const void* p : in)
    if (!p) return "null pointer";
  if ((uint64_t)W * H == 0 || scaled_too_large(W, H, scale)) return "bad frame size";
  return nullptr;
}
}  // namespace

int wpt_upsample(uint32_t scale, uint32_t sample, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags,
                 float* rgb3, uint8_t* valid, uint8_t* rgba) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = upsample_args(scale, iterations, sigma_c, sigma_z, flags, WPT_UPSAMPLE_MERGED))
    return fail(WPT_ERR_INVALID_ARG, e);
  if (scaled_too_large(g_session->renderer.width(), g_session->renderer.height(), scale))
    return fail(WPT_ERR_INVALID_ARG, "upsample: the scaled viewport has 2^32 pixels or more");
  if ((flags & WPT_UPSAMPLE_MERGED) && !g_session->renderer.has_merged())
    return fail(WPT_ERR_INVALID_ARG, "upsample: no wpt_reproject since the viewport was set");
  std::string err;
  if (!g_session->renderer.upsample(scale, sample, iterations, sigma_c, sigma_z, flags, rgb3, valid, rgba, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_upsample_planes(uint32_t W, uint32_t H, uint32_t scale, const float* acc3, const uint32_t* cnt, const float* t,
                        const float* normal3, const float* albedo3, const uint8_t* kind, const float* hi_t,
                        const float* hi_normal3, const float* hi_albedo3, const uint8_t* hi_kind,
                        const float* background3, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags,
                        float* rgb3, uint8_t* valid, uint8_t* rgba) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = upsample_args(scale, iterations, sigma_c, sigma_z, flags, 0u)) return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = upsample_plane_args(W, H, scale, {acc3, cnt, t, normal3, albedo3, kind, hi_t, hi_normal3,
                                                         hi_albedo3, hi_kind, background3}))
    return fail(WPT_ERR_INVALID_ARG, e);
  std::string err;
  Renderer& r = g_session->renderer;
  Guides lo, hi;
  lo.t = t; lo.normal = normal3; lo.albedo = albedo3; lo.kind = kind;
  hi.t = hi_t; hi.normal = hi_normal3; hi.albedo = hi_albedo3; hi.kind = hi_kind;
  if (!r.post().upsample_planes(r.stream(), HostFrame{W, H, acc3, cnt, nullptr, background3}, lo, scale, hi,
                                DnParams{iterations, sigma_c, sigma_z, 0u}, PostOut{rgb3, valid, rgba}, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_upsample_host(uint32_t W, uint32_t H, uint32_t scale, const float* acc3, const uint32_t* cnt, const float* t,
                      const float* normal3, const float* albedo3, const uint8_t* kind, const float* hi_t,
                      const float* hi_normal3, const float* hi_albedo3, const uint8_t* hi_kind,
                      const float* background3, uint32_t iterations, float sigma_c, float sigma_z, uint32_t flags,
                      float* rgb3, uint8_t* valid, uint8_t* rgba) {
  if (const char* e = upsample_args(scale, iterations, sigma_c, sigma_z, flags, 0u)) return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = upsample_plane_args(W, H, scale, {acc3, cnt, t, normal3, albedo3, kind, hi_t, hi_normal3,
                                                         hi_albedo3, hi_kind, background3}))
    return fail(WPT_ERR_INVALID_ARG, e);
  if (!rgb3 && !valid && !rgba) return WPT_OK;
  upsample_host(W, H, scale, acc3, cnt, t, normal3, albedo3, kind, hi_t, hi_normal3, hi_albedo3, hi_kind, background3,
                iterations, sigma_c, sigma_z, rgb3, valid, rgba);
  return WPT_OK;
}

int wpt_reproject_planes(uint32_t W, uint32_t H, const float* cam3, const float* acc3, const uint32_t* cnt,
                         const float* dir3, const float* t, const int32_t* id, const float* normal3,
                         const uint8_t* kind, const float* prev_cam5, const float* h_acc3, const uint32_t* h_cnt,
                         const float* h_t, const int32_t* h_id, const float* h_normal3, const uint8_t* h_kind,
                         float cos_min, float eps_z, uint32_t max_len, uint32_t flags, float* acc3_out,
                         uint32_t* cnt_out, uint32_t* len_out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = reproject_args(cos_min, eps_z, max_len, flags, kRpPlaneFlags)) return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = reproject_plane_args(W, H, {cam3, acc3, cnt, dir3, t, id, normal3, kind, prev_cam5, h_acc3, h_cnt,
                                                  h_t, h_id, h_normal3, h_kind}))
    return fail(WPT_ERR_INVALID_ARG, e);
  std::string err;
  Renderer& r = g_session->renderer;
  Guides g, hg;
  g.dir = dir3; g.t = t; g.id = id; g.normal = normal3; g.kind = kind;
  hg.t = h_t; hg.id = h_id; hg.normal = h_normal3; hg.kind = h_kind;
  if (!r.post().reproject_planes(r.stream(), HostFrame{W, H, acc3, cnt, cam3}, g, HostFrame{W, H, h_acc3, h_cnt, prev_cam5},
                                 hg, RpTest{cos_min, eps_z, max_len, flags}, RpHostOut{acc3_out, cnt_out, len_out}, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_reproject_host(uint32_t W, uint32_t H, const float* cam3, const float* acc3, const uint32_t* cnt,
                       const float* dir3, const float* t, const int32_t* id, const float* normal3, const uint8_t* kind,
                       const float* prev_cam5, const float* h_acc3, const uint32_t* h_cnt, const float* h_t,
                       const int32_t* h_id, const float* h_normal3, const uint8_t* h_kind, float cos_min, float eps_z,
                       uint32_t max_len, uint32_t flags, float* acc3_out, uint32_t* cnt_out, uint32_t* len_out) {
  if (const char* e = reproject_args(cos_min, eps_z, max_len, flags, kRpPlaneFlags)) return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = reproject_plane_args(W, H, {cam3, acc3, cnt, dir3, t, id, normal3, kind, prev_cam5, h_acc3, h_cnt,
                                                  h_t, h_id, h_normal3, h_kind}))
    return fail(WPT_ERR_INVALID_ARG, e);
  reproject_host(W, H, cam3, acc3, cnt, dir3, t, id, normal3, kind, prev_cam5, h_acc3, h_cnt, h_t, h_id, h_normal3,
                 h_kind, cos_min, eps_z, max_len, flags, acc3_out, cnt_out, len_out);
  return WPT_OK;
}

namespace {
// the argument rules the sample map's entry points share
const char* sample_map_args(uint32_t target, uint32_t max_per_pixel, uint32_t flags) {
  if (target == 0) return "sample_map: target must be > 0";
  if (max_per_pixel == 0) return "sample_map: max_per_pixel must be > 0";
  if (flags & ~(uint32_t)WPT_MAP_MISS_ONCE) return "sample_map: unknown flag";
  return nullptr;
}
const char* sample_map_plane_args(uint32_t W, uint32_t H, std::initializer_list<const void*> in) {
  for (const void* p : in)
    if (!p) return "null pointer";
  if ((uint64_t)W * H == 0 || (uint64_t)W * H >= 0xFFFFFFFFull) return "bad frame size";
  return nullptr;
}
}  // namespace

int wpt_sample_map(uint32_t sample, uint32_t target, uint32_t max_per_pixel, uint32_t budget, uint32_t flags,
                   uint32_t* count_out, uint64_t* total_out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = sample_map_args(target, max_per_pixel, flags)) return fail(WPT_ERR_INVALID_ARG, e);
  std::string err;
  bool invalid = false;
  if (!g_session->renderer.sample_map(sample, target, max_per_pixel, budget, flags, count_out, total_out, invalid, err))
    return fail(invalid ? WPT_ERR_INVALID_ARG : WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_sample_map_planes(uint32_t W, uint32_t H, const uint32_t* cnt, const uint32_t* len, const uint8_t* kind,
                          const uint8_t* member, uint32_t target, uint32_t max_per_pixel, uint32_t budget,
                          uint32_t flags, uint32_t* count_out, uint64_t* total_out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = sample_map_args(target, max_per_pixel, flags)) return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = sample_map_plane_args(W, H, {cnt, len, kind, member})) return fail(WPT_ERR_INVALID_ARG, e);
  std::string err;
  bool invalid = false;
  Renderer& r = g_session->renderer;
  if (!r.post().sample_map_planes(r.stream(), MapPlanes{(uint32_t)((size_t)W * H), cnt, len, kind, member},
                                  MapParams{target, max_per_pixel, budget, flags}, MapOut{count_out, total_out}, invalid,
                                  err))
    return fail(invalid ? WPT_ERR_INVALID_ARG : WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_sample_map_host(uint32_t W, uint32_t H, const uint32_t* cnt, const uint32_t* len, const uint8_t* kind,
                        const uint8_t* member, uint32_t target, uint32_t max_per_pixel, uint32_t budget, uint32_t flags,
                        uint32_t* count_out, uint64_t* total_out) {
  if (const char* e = sample_map_args(target, max_per_pixel, flags)) return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = sample_map_plane_args(W, H, {cnt, len, kind, member})) return fail(WPT_ERR_INVALID_ARG, e);
  if (!sample_map_host(W, H, cnt, len, kind, member, target, max_per_pixel, budget, flags, count_out, total_out))
    return fail(WPT_ERR_INVALID_ARG, "sample_map: the needs sum to 2^32 or more (lower max_per_pixel)");
  return WPT_OK;
}

int wpt_compute_map(const uint32_t* count) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  bool invalid = false;
  if (!g_session->renderer.compute_map(count, invalid, err))
    return fail(invalid ? WPT_ERR_INVALID_ARG : WPT_ERR_DEVICE, err);
  return WPT_OK;
}

namespace {
// the argument rules of wpt_radiance_rays
const char* radiance_rays_args(size_t n, const float* rays6, uint32_t sample, uint32_t spp, uint32_t type,
                               uint32_t flags, const float* rgb3) {
  if (n && (!rays6 || !rgb3)) return "radiance_rays: null rays6 or rgb3";
  if (spp == 0) return "radiance_rays: spp 0";
  if (type > 2) return "radiance_rays: Invalid RenderType magic number";
  if (flags & ~(uint32_t)WPT_RAYS_DEVICE) return "radiance_rays: unknown flag";
  if ((uint64_t)sample + spp - 1 > 0xFFFFFFFFull) return "radiance_rays: a sample index would pass 2^32 - 1";
  if ((uint64_t)n >= (1ull << 32)) return "radiance_rays: 2^32 rays or more";
  return nullptr;
}
}  // namespace

int wpt_radiance_rays(size_t n, const float* rays6, const uint32_t* keys, uint32_t sample, uint32_t spp, uint32_t type,
                      uint32_t flags, float* rgb3, uint8_t* status) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (const char* e = radiance_rays_args(n, rays6, sample, spp, type, flags, rgb3)) return fail(WPT_ERR_INVALID_ARG, e);
  std::string err;
  if (!g_session->renderer.radiance_rays(n, rays6, keys, sample, spp, type, (flags & WPT_RAYS_DEVICE) != 0, rgb3, status,
                                         err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_first_hit_rays(size_t n, const float* rays6, uint32_t flags, float* t, int32_t* id, uint32_t* visits,
                       float* normal3, float* albedo3, uint8_t* kind, uint8_t* status) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  const bool wanted = t || id || visits || normal3 || albedo3 || kind || status;
  if (flags & ~(uint32_t)WPT_RAYS_DEVICE) return fail(WPT_ERR_INVALID_ARG, "first_hit_rays: unknown flag");
  if ((uint64_t)n >= (1ull << 32)) return fail(WPT_ERR_INVALID_ARG, "first_hit_rays: 2^32 rays or more");
  if (n && wanted && !rays6) return fail(WPT_ERR_INVALID_ARG, "first_hit_rays: null rays6");
  std::string err;
  if (!g_session->renderer.first_hit_rays(n, rays6, (flags & WPT_RAYS_DEVICE) != 0, t, id, visits, normal3, albedo3, kind,
                                          status, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_denoise_rays(uint32_t W, uint32_t H, const float* rays6, const uint32_t* keys, uint32_t sample, uint32_t spp,
                     uint32_t type, uint32_t iterations, float sigma_c, float sigma_z, uint32_t dn_flags, uint32_t flags,
                     float* rgb3, uint8_t* valid, uint8_t* rgba, float* raw3, uint8_t* status) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  const uint64_t n = (uint64_t)W * H;
  if (n == 0 || n >= (1ull << 32)) return fail(WPT_ERR_INVALID_ARG, "denoise_rays: W * H is 0, or 2^32 or more");
  // radiance_rays' rules (its rgb3 may be null here: raw3 is one output of five)
  const float nonnull = 0.0f;
  if (const char* e = radiance_rays_args((size_t)n, rays6, sample, spp, type, flags, &nonnull))
    return fail(WPT_ERR_INVALID_ARG, e);
  if (const char* e = denoise_args(iterations, sigma_c, sigma_z, dn_flags)) return fail(WPT_ERR_INVALID_ARG, e);
  std::string err;
  if (!g_session->renderer.denoise_rays(W, H, rays6, keys, sample, spp, type,
                                        DnParams{iterations, sigma_c, sigma_z, dn_flags},
                                        (flags & WPT_RAYS_DEVICE) != 0, rgb3, valid, rgba, raw3, status, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_rays_valid(size_t n, const float* rays6, uint8_t* status) {
  if (n && (!rays6 || !status)) return fail(WPT_ERR_INVALID_ARG, "null argument");
  for (size_t i = 0; i < n; i++) status[i] = ray_valid(rays6 + 6 * i) ? 1 : 0;
  return WPT_OK;
}

int wpt_radiance_points(size_t n, const float* points6, const uint32_t* keys, uint32_t sample, uint32_t spp,
                        uint32_t type, uint32_t dist, uint32_t flags, float* rgb3, uint8_t* status) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  // radiance_rays' rules on the records, and the distribution
  if (const char* e = radiance_rays_args(n, points6, sample, spp, type, flags, rgb3)) return fail(WPT_ERR_INVALID_ARG, e);
  if (dist > WPT_POINTS_SPHERE) return fail(WPT_ERR_INVALID_ARG, "radiance_points: unknown distribution");
  std::string err;
  if (!g_session->renderer.radiance_points(n, points6, keys, sample, spp, type, dist, (flags & WPT_RAYS_DEVICE) != 0,
                                           rgb3, status, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

// point_ray (wpt_points.h) on the host: the generators' own code
int wpt_point_rays(size_t n, const float* points6, const uint32_t* keys, uint32_t frame_seed, uint32_t sample,
                   uint32_t dist, float* rays6) {
  if (n && (!points6 || !rays6)) return fail(WPT_ERR_INVALID_ARG, "null argument");
  if (dist > WPT_POINTS_SPHERE) return fail(WPT_ERR_INVALID_ARG, "point_rays: unknown distribution");
  for (size_t i = 0; i < n; i++) {
    V3 o = mk(0.0f, 0.0f, 0.0f), wi = o;
    uint32_t st = 0;
    point_ray(points6 + 6 * i, keys ? keys[i] : (uint32_t)i, frame_seed, sample, dist, o, wi, st);
    float* r = rays6 + 6 * i;
    r[0] = o.x; r[1] = o.y; r[2] = o.z;
    r[3] = wi.x; r[4] = wi.y; r[5] = wi.z;
  }
  return WPT_OK;
}

static_assert(WPT_SH_MAX_ORDER == kShMaxOrder && WPT_SH_CHUNK == kShQueryChunk, "the header's SH constants");

int wpt_probe_sh(size_t n, const float* points6, const uint32_t* keys, uint32_t sample, uint32_t spp, uint32_t type,
                 uint32_t dist, uint32_t order, uint32_t flags, float* sh, uint8_t* status) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  // radiance_points' rules, and the order
  if (const char* e = radiance_rays_args(n, points6, sample, spp, type, flags, sh)) return fail(WPT_ERR_INVALID_ARG, e);
  if (dist > WPT_POINTS_SPHERE) return fail(WPT_ERR_INVALID_ARG, "probe_sh: unknown distribution");
  if (order > WPT_SH_MAX_ORDER) return fail(WPT_ERR_INVALID_ARG, "probe_sh: order above WPT_SH_MAX_ORDER");
  std::string err;
  if (!g_session->renderer.probe_sh(n, points6, keys, sample, spp, type, dist, order, (flags & WPT_RAYS_DEVICE) != 0, sh,
                                    status, err))
    return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

// sh_basis (wpt_sh.h) on the host: the kernel's own code
int wpt_sh_basis(size_t n, const float* dirs3, uint32_t order, float* out) {
  if (n && (!dirs3 || !out)) return fail(WPT_ERR_INVALID_ARG, "null argument");
  if (order > WPT_SH_MAX_ORDER) return fail(WPT_ERR_INVALID_ARG, "sh_basis: order above WPT_SH_MAX_ORDER");
  sh_basis_rows(n, dirs3, order, out);
  return WPT_OK;
}

int wpt_presolve_rays(size_t n, const float* rays, uint8_t* resolved, float* t_out, int32_t* id_out) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (n && (!rays || !resolved || !t_out || !id_out)) return fail(WPT_ERR_INVALID_ARG, "null argument");
  std::string err;
  if (!g_session->renderer.presolve_rays(n, rays, resolved, t_out, id_out, err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_presolve_shadow_rays(size_t n, const float* pq, const int32_t* light, uint8_t* resolved) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  if (n && (!pq || !light || !resolved)) return fail(WPT_ERR_INVALID_ARG, "null argument");
  std::string err;
  if (!g_session->renderer.presolve_shadow_rays(n, pq, light, resolved, err)) return fail(WPT_ERR_DEVICE, err);
  return WPT_OK;
}

int wpt_shadow_rays(size_t n, const float* pq, const int32_t* light, uint8_t* occluded) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  std::string err;
  if (!g_session->renderer.shadow_rays(n, pq, light, occluded, err)) return fail(WPT_ERR_INVALID_ARG, err);
  return WPT_OK;
}

int wpt_shutdown(void) {
  if (!g_session) return fail(WPT_ERR_NOT_INIT, "init not called");
  delete g_session;
  g_session = nullptr;
  return WPT_OK;
}

// ---- host-only inspection ---------------------------------------------------
void* wpt_debug_scene_new(int32_t scene_id, const float* mesh_vertices, size_t num_vertices) {
  std::vector<float> mesh;
  if (mesh_vertices && num_vertices) mesh.assign(mesh_vertices, mesh_vertices + ((num_vertices / 3) * 9));
  HostScene* sc = new HostScene();
  std::string err;
  if (!build_scene(scene_id, mesh, *sc, err)) {
    delete sc;
    fail(WPT_ERR_INVALID_SCENE, err);
    return nullptr;
  }
  return sc;
}

void* wpt_debug_scene_new_gpu(int32_t scene_id, const float* mesh_vertices, size_t num_vertices) {
  // one builder for the process, on the device wpt_set_device chose; never
  // freed (its buffers would outlive the HIP runtime at exit)
  static BvhGpu* gpu = nullptr;
  const hipError_t he = hipSetDevice(g_device);
  if (he != hipSuccess) {
    fail(WPT_ERR_DEVICE, std::string("hipSetDevice failed: ") + hipGetErrorString(he));
    return nullptr;
  }
  if (!gpu) gpu = new BvhGpu();
  gpu->min_shapes = 0;
  std::vector<float> mesh;
  if (mesh_vertices && num_vertices) mesh.assign(mesh_vertices, mesh_vertices + ((num_vertices / 3) * 9));
  HostScene* sc = new HostScene();
  std::string err;
  if (!build_scene(scene_id, mesh, *sc, err, gpu)) {
    delete sc;
    fail(err.rfind("HIP error", 0) == 0 || err.rfind("GPU BVH", 0) == 0 ? WPT_ERR_DEVICE : WPT_ERR_INVALID_SCENE,
         err);
    return nullptr;
  }
  return sc;
}

int wpt_debug_scene_build_info(void* h, double* out) {
  if (!h || !out) return fail(WPT_ERR_INVALID_ARG, "null argument");
  const HostScene* sc = (const HostScene*)h;
  out[0] = sc->bvh_ms;
  out[1] = sc->bvh_on_gpu ? 1.0 : 0.0;
  return WPT_OK;
}

int wpt_debug_scene_info(void* h, uint64_t* out) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc) return fail(WPT_ERR_INVALID_ARG, "null scene");
  uint64_t v[8] = {sc->shapes.size(), sc->num_inf, sc->nodes.size(), sc->lights.size(), sc->depth,
                   sc->use_bvh ? 1u : 0u, sc->tri_only ? 1u : 0u, sc->nodes4.size()};
  memcpy(out, v, sizeof v);
  return WPT_OK;
}

int wpt_debug_scene_nodes(void* h, uint32_t* out) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc) return fail(WPT_ERR_INVALID_ARG, "null scene");
  for (size_t i = 0; i < sc->nodes.size(); i++) {
    const Node2& n = sc->nodes[i];
    float b[6] = {n.bmin[0], n.bmin[1], n.bmin[2], n.bmax[0], n.bmax[1], n.bmax[2]};
    memcpy(out + 8 * i, b, sizeof b);
    out[8 * i + 6] = n.left_first;
    out[8 * i + 7] = n.count;
  }
  return WPT_OK;
}

int wpt_debug_scene_nodes4(void* h, uint32_t* out) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc) return fail(WPT_ERR_INVALID_ARG, "null scene");
  for (size_t i = 0; i < sc->nodes4.size(); i++) {
    const Node4& n = sc->nodes4[i];
    uint32_t* o = out + 37 * i;
    memset(o, 0, 37 * sizeof(uint32_t));
    for (int k = 0; k < 4; k++) {
      const uint32_t c = n.child[k];
      if (c == kChildEmpty) continue;
      o[0]++;
      uint32_t* e = o + 1 + 9 * k;
      if (!(c & 0x80000000u)) {
        e[0] = 1;
        e[1] = c;
      } else {
        e[0] = 2;
        if ((c & 0xC0000000u) == 0xC0000000u) {
          e[1] = sc->leaf_table[2 * (c & 0x3FFFFFFFu)];
          e[2] = sc->leaf_table[2 * (c & 0x3FFFFFFFu) + 1];
        } else {
          e[1] = c & 0xFFFFFFu;
          e[2] = (c >> 24) & 0x3Fu;
        }
      }
      const float b[6] = {n.xmin[k], n.ymin[k], n.zmin[k], n.xmax[k], n.ymax[k], n.zmax[k]};
      memcpy(e + 3, b, sizeof b);
    }
  }
  return WPT_OK;
}

int wpt_debug_scene_shapes(void* h, float* out) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc) return fail(WPT_ERR_INVALID_ARG, "null scene");
  for (size_t i = 0; i < sc->shapes.size(); i++) {
    const Shape& s = sc->shapes[i];
    float* o = out + 16 * i;
    memcpy(o, s.g, sizeof s.g);
    o[12] = (float)s.kind;
    o[13] = s.emissive ? 1.0f : 0.0f;
    o[14] = 0.0f;
    o[15] = 0.0f;
  }
  return WPT_OK;
}

int wpt_debug_scene_materials(void* h, float* out) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc || !out) return fail(WPT_ERR_INVALID_ARG, "null argument");
  for (size_t i = 0; i < sc->shapes.size(); i++) {
    const Shape& s = sc->shapes[i];
    float* o = out + 4 * i;
    memcpy(o, s.m, sizeof s.m);
    o[3] = s.emissive ? 1.0f : 0.0f;
  }
  return WPT_OK;
}

int wpt_debug_scene_lights(void* h, uint32_t* out) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc) return fail(WPT_ERR_INVALID_ARG, "null scene");
  for (size_t i = 0; i < sc->lights.size(); i++) out[i] = sc->lights[i];
  return WPT_OK;
}

int wpt_debug_scene_presolve(void* h, size_t n, const float* rays, uint8_t* resolved, float* t_out, int32_t* id_out) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc || (n && (!rays || !resolved || !t_out || !id_out))) return fail(WPT_ERR_INVALID_ARG, "null argument");
  // the host restatement: the same presolve_ray over the scene's planes as
  // upload_scene lays them out (normal, normal . location)
  HostPlanes hp{};
  hp.num_inf = 0;
  PresolveBoxes pre{};
  if (sc->use_bvh && sc->shapes.size() > sc->num_inf && sc->num_inf <= 16) {
    pre = sc->pre;
    hp.num_inf = sc->num_inf;
    for (uint32_t i = 0; i < sc->num_inf; i++) {
      const float* g = sc->shapes[i].g;
      const V3 loc = mk(g[0], g[1], g[2]), nrm = mk(g[3], g[4], g[5]);
      hp.planes[i] = HostPlanes::P4{nrm.x, nrm.y, nrm.z, dot(nrm, loc)};
    }
  }
  for (size_t i = 0; i < n; i++) {
    const float* r = rays + 6 * i;
    resolved[i] = presolve_ray(hp, pre, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), t_out[i], id_out[i]) ? 1 : 0;
  }
  return WPT_OK;
}

// The host's planes and presolve data of a scene, as upload_scene lays them
// out (planes: normal, normal . location).
static void host_presolve_view(const HostScene* sc, HostPlanes& hp, PresolveBoxes& pre) {
  hp = HostPlanes{};
  pre = PresolveBoxes{};
  if (sc->use_bvh && sc->shapes.size() > sc->num_inf && sc->num_inf <= 16) {
    pre = sc->pre;
    hp.num_inf = sc->num_inf;
    for (uint32_t i = 0; i < sc->num_inf; i++) {
      const float* g = sc->shapes[i].g;
      const V3 loc = mk(g[0], g[1], g[2]), nrm = mk(g[3], g[4], g[5]);
      hp.planes[i] = HostPlanes::P4{nrm.x, nrm.y, nrm.z, dot(nrm, loc)};
    }
  }
}

int wpt_debug_scene_presolve_shadow(void* h, size_t n, const float* pq, const int32_t* light, uint8_t* resolved) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc || (n && (!pq || !light || !resolved))) return fail(WPT_ERR_INVALID_ARG, "null argument");
  // the host restatement: the same presolve_shadow on the operands
  // shade_path derives from {p, q} (shadow_operands)
  HostPlanes hp;
  PresolveBoxes pre;
  host_presolve_view(sc, hp, pre);
  for (size_t i = 0; i < n; i++) {
    const float* r = pq + 6 * i;
    V3 o, d;
    float dl;
    shadow_operands(mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), o, d, dl);
    resolved[i] = presolve_shadow(hp, pre, o, d, dl, light[i]) ? 1 : 0;
  }
  return WPT_OK;
}

int wpt_debug_scene_guard_lights(void* h, uint32_t* light_guards, uint32_t* num, int32_t* ids) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc || !light_guards || !num) return fail(WPT_ERR_INVALID_ARG, "null argument");
  *light_guards = sc->pre.light_guards;
  *num = sc->pre.num_guard_lights;
  if (ids)
    for (int k = 0; k < kMaxGuardLights; k++) ids[k] = (uint32_t)k < sc->pre.num_guard_lights ? sc->pre.guard_light_id[k] : -1;
  return WPT_OK;
}

int wpt_debug_scene_guards(void* h, uint32_t* num_guards, float* boxes, uint32_t* leaf_guard) {
  const HostScene* sc = (const HostScene*)h;
  if (!sc || !num_guards) return fail(WPT_ERR_INVALID_ARG, "null argument");
  *num_guards = sc->pre.num_guards;
  if (boxes) {
    memcpy(boxes, sc->pre.root, 6 * sizeof(float));
    memcpy(boxes + 6, sc->pre.guard, 6 * kMaxGuards * sizeof(float));
  }
  if (leaf_guard)
    for (size_t i = 0; i < sc->nodes.size(); i++) leaf_guard[i] = i < sc->leaf_guard.size() ? sc->leaf_guard[i] : ~0u;
  return WPT_OK;
}

void wpt_debug_scene_free(void* h) { delete (HostScene*)h; }

}  // extern "C"
