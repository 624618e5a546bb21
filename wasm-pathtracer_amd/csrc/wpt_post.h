// wpt_post.h — frame post-processing: what runs on a frame after it was traced
// and never touches a path, a lane, a batch or the BVH. The a-trous filter
// (wpt_denoise.h), the reprojection of a kept history (wpt_reproject.h), the
// guided upsampling (wpt_upsample.h) and the planning of a sample map
// (wpt_guided.h): their kernels, their scratch layouts and the state they keep
// between calls, in wpt_post.hip.
//
// A FramePost is told everything of the session it needs by value: the frame
// (FrameRef, which carries the stream), first-hit guide planes (Guides, made by
// Renderer::first_hit_launch) and the call's parameters. The *_planes test
// hooks take a caller's host planes and a stream, nothing of a session.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "wpt_devmem.h"

namespace wpt {

// First-hit planes of one viewport (wpt_first_hit's: dir, normal and albedo 3
// floats per pixel); a plane not wanted is null. Device pointers, or a hook's
// host planes before upload_guides.
struct Guides {
  const float* dir = nullptr;
  const float* t = nullptr;
  const int32_t* id = nullptr;
  const float* normal = nullptr;
  const float* albedo = nullptr;
  const uint8_t* kind = nullptr;
};

// A frame on the device as the session holds it: the sums and counts, the
// camera (5 floats) and the scene's background (3) on the host, the
// accumulation's epoch (Renderer::reset counts them) and the stream every step
// is queued on.
struct FrameRef {
  uint32_t W = 0, H = 0;
  const float4* acc = nullptr;
  const uint32_t* cnt = nullptr;
  const float* cam = nullptr;
  const float* bg = nullptr;
  uint64_t epoch = 0;
  hipStream_t stream = nullptr;
};

// A hook's frame on the host: rgb sums; cam and bg where the operation reads
// them (reproject_planes: the camera's position, for the history's frame the 5
// floats of the previous camera; upsample_planes: the background).
struct HostFrame {
  uint32_t W = 0, H = 0;
  const float* acc3 = nullptr;
  const uint32_t* cnt = nullptr;
  const float* cam = nullptr;
  const float* bg = nullptr;
};

struct DnParams {  // the filter's (wpt_denoise)
  uint32_t iterations;
  float sigma_c, sigma_z;
  uint32_t flags;
};
struct PostOut {  // the filter's and the upsampling's host outputs; a null one is not written
  float* rgb3;
  uint8_t* valid;
  uint8_t* rgba;
};
struct RpTest {  // the reprojection's tests and flags (wpt_reproject)
  float cos_min, eps_z;
  uint32_t max_len, flags;
};
struct RpHostOut {  // its host outputs; a null one is not written
  float* acc3;
  uint32_t* cnt;
  uint32_t* len;
};
struct MapPlanes {  // sample_map's inputs over np pixels (null len / kind / member: see k_map_need)
  uint32_t np;
  const uint32_t* cnt;
  const uint32_t* len;
  const uint8_t* kind;
  const uint8_t* member;
};
struct MapParams {  // (wpt_sample_map)
  uint32_t target, max_pp, budget, flags;
};
struct MapOut {  // the map (np counts) and {T, dealt} on the host; a null one is not written
  uint32_t* count;
  uint64_t* total;
};

class FramePost {
 public:
  // The session's calls (Renderer checks the scene and the viewport and makes
  // the guides). Everything is queued on F.stream, neither timed nor counted,
  // and waited for; the frame is only read.
  //
  // the a-trous filter on the frame under guides t, normal, albedo, kind. The
  // frame need not be the session's (wpt_denoise_rays hands in a query's sums
  // and counts: F.cam is not read): the scratch grows to the frame at hand and
  // is still freed with the viewport. dev_out: O's are device pointers.
  bool denoise(const FrameRef& F, const Guides& g, const DnParams& P, const PostOut& O, std::string& err,
               bool dev_out = false);
  // the same over the merged frame and the guides the last reproject left
  bool denoise_merged(const FrameRef& F, const DnParams& P, const PostOut& O, std::string& err);
  // the kept history into the frame's camera, merged with the frame; the merged
  // frame and the guides stay on the device. kRpKeep: they, and the camera,
  // become the history (g.id is then needed, as under kRpSameShape with a history)
  bool reproject(const FrameRef& F, const Guides& g, const RpTest& T, const RpHostOut& O, std::string& err);
  // the filter's pack and passes on the frame under `lo` (null: on the merged
  // frame and its guides), then k_upsample to scale times the viewport under
  // the fine guides `hi`
  bool upsample(const FrameRef& F, const Guides* lo, uint32_t scale, const Guides& hi, const DnParams& P,
                const PostOut& O, std::string& err);
  // the map planned from the frame's counts, the len plane of this epoch's last
  // reproject and `kind` (device, null unless kMapMissOnce); member: the
  // partition's pixels on the host (null: every pixel). The map stays on the
  // device for map_counts. `invalid`: the failure is the caller's argument.
  bool sample_map(const FrameRef& F, const uint8_t* kind, const std::vector<uint8_t>* member, const MapParams& P,
                  const MapOut& O, bool& invalid, std::string& err);

  // Test hooks: the same kernels and launch geometry on a caller's host planes,
  // in buffers of their own; the state below is not touched.
  bool denoise_planes(hipStream_t s, const HostFrame& F, const Guides& g, const DnParams& P, const PostOut& O,
                      std::string& err);
  bool reproject_planes(hipStream_t s, const HostFrame& F, const Guides& g, const HostFrame& hist, const Guides& hg,
                        const RpTest& T, const RpHostOut& O, std::string& err);
  bool upsample_planes(hipStream_t s, const HostFrame& F, const Guides& lo, uint32_t scale, const Guides& hi,
                       const DnParams& P, const PostOut& O, std::string& err);
  bool sample_map_planes(hipStream_t s, const MapPlanes& in, const MapParams& P, const MapOut& O, bool& invalid,
                         std::string& err);

  // a merged frame of this viewport is on the device (denoise_merged, kUpMerged)
  bool has_merged() const { return rp_merged_; }
  // WPT_OPT_HISTORY: 0 no history, 1 usable, 2 kept in accumulation `epoch`
  int history_state(uint64_t epoch) const { return hist_cur_ < 0 ? 0 : hist_epoch_ == epoch ? 2 : 1; }
  void history_drop() { hist_cur_ = -1; }
  // the counts of the map sample_map planned in accumulation `epoch` for a
  // frame of np pixels (device), or null if there is none
  const uint32_t* map_counts(uint64_t epoch, size_t np) const;
  uint32_t dn_lds() const { return dn_lds_; }
  void set_dn_lds(uint32_t mask) { dn_lds_ = mask; }
  // Frees (and so synchronises the device) what was made on first use since:
  // with the viewport the filter's and the upsampling's scratch, both kept
  // frames and the merged frame; with the partition the sample map.
  enum class Sized { kViewport, kPartition };
  void release(Sized by);

 private:
  // The filter's scratch for the session's viewport (records A0, A1, B, a' and
  // the outputs) and the upsampling's outputs.
  DevBuf<char> d_dn_;
  DevBuf<char> d_up_;
  uint32_t dn_lds_ = 7;  // WPT_OPT_DENOISE_LDS: iteration i runs the LDS kernel if bit i is set
  // Reprojection. A history kept at the current epoch already holds the current
  // samples. d_hist_: the two kept frames, ping-ponged (a keeping call reads
  // one and writes the other), hist_cur_ the live one or -1, hist_cam_ its
  // camera; d_rp_: the merged frame and the guide planes of the last call,
  // there while rp_merged_, its len plane of accumulation rp_epoch_
  // (sample_map reads it in that one only).
  DevBuf<char> d_hist_[2];
  DevBuf<char> d_rp_;
  int hist_cur_ = -1;
  uint64_t hist_epoch_ = 0;
  float hist_cam_[5] = {0, 0, 0, 0, 0};
  bool rp_merged_ = false;
  uint64_t rp_epoch_ = 0;
  // Guided sampling. d_map_: sample_map's scratch and the map it leaves, valid
  // in accumulation map_epoch_ while map_ok_.
  DevBuf<char> d_map_;
  bool map_ok_ = false;
  uint64_t map_epoch_ = 0;
};

}  // namespace wpt
