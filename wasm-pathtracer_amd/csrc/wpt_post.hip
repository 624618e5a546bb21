// wpt_post.hip — frame post-processing (wpt_post.h): the kernels of the a-trous
// filter, the reprojection, the guided upsampling and the sample map's
// planning, the layouts of their scratch, and FramePost's host side. Compiled
// with wpt_render.hip's flags: the kernels are the ones that unit held.
#include "wpt_post.h"
#include "wpt_launch.h"

#include <cstring>

namespace wpt {

namespace {

#define WPT_DENOISE_KERNELS
#include "wpt_denoise.h"
#define WPT_REPROJECT_KERNELS
#include "wpt_reproject.h"
#define WPT_GUIDED_KERNELS
#include "wpt_guided.h"
#define WPT_UPSAMPLE_KERNELS
#include "wpt_upsample.h"

// ---------------------------------------------------------------------------
// Scratch layouts: parts of np pixels, each 256 B aligned (Slices)
// ---------------------------------------------------------------------------

// The filter's scratch: the records A0, A1 and B, a', then the outputs rgb,
// rgba and valid.
struct DnLayout {
  size_t a0 = 0, a1 = 0, b = 0, ap = 0, rgb = 0, rgba = 0, valid = 0, bytes = 0;
  constexpr explicit DnLayout(size_t np) {
    Slices z;
    a0 = z.take(16 * np); a1 = z.take(16 * np); b = z.take(16 * np); ap = z.take(12 * np); rgb = z.take(12 * np);
    rgba = z.take(4 * np); valid = z.take(np);
    bytes = z.at;
  }
};
static_assert(DnLayout(1000).bytes == 77568 && DnLayout(1000).valid == 76544 && DnLayout(1000).ap == 48384,
              "denoise's layout");

// A kept frame's planes, and the merged frame with the guide planes the filter reads.
struct RpHistLayout {
  size_t k = 0, r0 = 0, r1 = 0, id = 0, bytes = 0;
  constexpr explicit RpHistLayout(size_t np) {
    Slices z;
    r0 = z.take(16 * np); r1 = z.take(16 * np); k = z.take(4 * np); id = z.take(4 * np);
    bytes = z.at;
  }
  RpHist at(void* base) const {
    char* b = (char*)base;
    RpHist h;
    h.k = (uint32_t*)(b + k); h.r0 = (float4*)(b + r0); h.r1 = (float4*)(b + r1); h.id = (int32_t*)(b + id);
    return h;
  }
};
static_assert(RpHistLayout(1000).bytes == 40448 && RpHistLayout(1000).k == 32256 && RpHistLayout(1000).id == 36352,
              "the kept frame's layout");
struct RpMerged {
  float4* acc;
  uint32_t* cnt;
  uint32_t* len;
  float* t;
  float* normal;
  float* albedo;
  uint8_t* kind;
  Guides guides() const {
    Guides g;
    g.t = t; g.normal = normal; g.albedo = albedo; g.kind = kind;
    return g;
  }
};
struct RpMergedLayout {
  size_t acc = 0, cnt = 0, len = 0, t = 0, normal = 0, albedo = 0, kind = 0, bytes = 0;
  constexpr explicit RpMergedLayout(size_t np) {
    Slices z;
    acc = z.take(16 * np); cnt = z.take(4 * np); len = z.take(4 * np); t = z.take(4 * np); normal = z.take(12 * np);
    albedo = z.take(12 * np); kind = z.take(np);
    bytes = z.at;
  }
  RpMerged at(void* base) const {
    char* m = (char*)base;
    return RpMerged{(float4*)(m + acc),   (uint32_t*)(m + cnt), (uint32_t*)(m + len), (float*)(m + t),
                    (float*)(m + normal), (float*)(m + albedo), (uint8_t*)(m + kind)};
  }
};
static_assert(RpMergedLayout(1000).bytes == 53504 && RpMergedLayout(1000).len == 20224 &&
                  RpMergedLayout(1000).kind == 52480,
              "the merged frame's layout");
const RpHist kNoHist = {nullptr, nullptr, nullptr, nullptr};

// The outputs of a fine frame of nf pixels.
struct UpLayout {
  size_t rgb = 0, rgba = 0, valid = 0, bytes = 0;
  constexpr explicit UpLayout(size_t nf) {
    Slices z;
    rgb = z.take(12 * nf); rgba = z.take(4 * nf); valid = z.take(nf);
    bytes = z.at;
  }
};
static_assert(UpLayout(1000).bytes == 17152 && UpLayout(1000).rgba == 12032 && UpLayout(1000).valid == 16128,
              "upsample's layout");

// sample_map's scratch: the needs and their scan (np + 1 u64), the chunk
// sums, the map itself and the membership plane
struct MapLayout {
  size_t pre = 0, sums = 0, count = 0, member = 0, bytes = 0;
  uint32_t nb = 0;
  constexpr explicit MapLayout(size_t np) {
    nb = (uint32_t)((np + 1 + kScanChunk - 1) / kScanChunk);
    Slices z;
    pre = z.take(8 * (np + 1)); sums = z.take(8 * ((size_t)nb + 1)); count = z.take(4 * np); member = z.take(np);
    bytes = z.at;
  }
};
// (scans in chunks of 1024: 5000 pixels are 5 chunks)
static_assert(kScanChunk == 1024 && MapLayout(5000).nb == 5 && MapLayout(5000).bytes == 65792 &&
                  MapLayout(5000).count == 40448 && MapLayout(5000).member == 60672,
              "sample_map's layout");

// ---------------------------------------------------------------------------
// What the calls share
// ---------------------------------------------------------------------------

bool wanted(const PostOut& O) { return O.rgb3 || O.valid || O.rgba; }

// The device outputs that were asked for (the null ones are not looked at) of
// n pixels to the host (dev_out: to the caller's device pointers), then waits
// for s.
bool copy_out(hipStream_t s, const PostOut& O, const PostOut& dev, size_t n, std::string& err, bool dev_out = false) {
  const hipMemcpyKind kind = dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (O.rgb3) HIP_OK(hipMemcpyAsync(O.rgb3, dev.rgb3, 12 * n, kind, s));
  if (O.valid) HIP_OK(hipMemcpyAsync(O.valid, dev.valid, n, kind, s));
  if (O.rgba) HIP_OK(hipMemcpyAsync(O.rgba, dev.rgba, 4 * n, kind, s));
  HIP_OK(hipStreamSynchronize(s));
  return true;
}

// A hook's host guide planes of n pixels into buffers of S, the uploads queued
// on s (the caller waits); a null plane stays null. After a failed allocation
// (S.ok false, which the caller reports) nothing is queued.
bool upload_guides(hipStream_t s, HookScratch& S, const Guides& h, size_t n, Guides& d, std::string& err) {
  float* dir = h.dir ? S.d<float>(3 * n) : nullptr;
  float* t = h.t ? S.d<float>(n) : nullptr;
  int32_t* id = h.id ? S.d<int32_t>(n) : nullptr;
  float* normal = h.normal ? S.d<float>(3 * n) : nullptr;
  float* albedo = h.albedo ? S.d<float>(3 * n) : nullptr;
  uint8_t* kind = h.kind ? S.d<uint8_t>(n) : nullptr;
  d.dir = dir; d.t = t; d.id = id; d.normal = normal; d.albedo = albedo; d.kind = kind;
  if (!S.ok) return true;
  if (dir) HIP_OK(hipMemcpyAsync(dir, h.dir, 12 * n, hipMemcpyHostToDevice, s));
  if (t) HIP_OK(hipMemcpyAsync(t, h.t, 4 * n, hipMemcpyHostToDevice, s));
  if (id) HIP_OK(hipMemcpyAsync(id, h.id, 4 * n, hipMemcpyHostToDevice, s));
  if (normal) HIP_OK(hipMemcpyAsync(normal, h.normal, 12 * n, hipMemcpyHostToDevice, s));
  if (albedo) HIP_OK(hipMemcpyAsync(albedo, h.albedo, 12 * n, hipMemcpyHostToDevice, s));
  if (kind) HIP_OK(hipMemcpyAsync(kind, h.kind, n, hipMemcpyHostToDevice, s));
  return true;
}

// A hook's frame: its sums as float4 and its counts into acc and cnt, queued
// like the guides (`stage` lives until the caller has waited).
bool upload_frame(hipStream_t s, const HostFrame& h, float4* acc, uint32_t* cnt, std::vector<float4>& stage,
                  FrameRef& F, std::string& err) {
  const size_t np = (size_t)h.W * h.H;
  HIP_OK(upload_rgb3(s, h.acc3, np, stage, acc));
  HIP_OK(hipMemcpyAsync(cnt, h.cnt, sizeof(uint32_t) * np, hipMemcpyHostToDevice, s));
  F.W = h.W; F.H = h.H;
  F.acc = acc; F.cnt = cnt;
  F.cam = h.cam; F.bg = h.bg;
  F.stream = s;
  return true;
}

// ---------------------------------------------------------------------------
// The a-trous filter (wpt_denoise.h)
// ---------------------------------------------------------------------------

template <int STEP>
void launch_atrous(bool lds, dim3 grid, hipStream_t s, const float4* A, const float4* B, uint32_t W, uint32_t H,
                   float s2, float sigma_z, float4* Aout) {
  if constexpr (STEP <= 4) {
    if (lds) {
      k_dn_atrous<STEP, true><<<grid, kBlock, 0, s>>>(A, B, W, H, s2, sigma_z, Aout);
      return;
    }
  }
  k_dn_atrous<STEP, false><<<grid, kBlock, 0, s>>>(A, B, W, H, s2, sigma_z, Aout);
}

// Pack and the iterations over device planes in a scratch of DnLayout(W * H),
// queued on F.stream; the filtered records come back as rec (beside B and a').
// Iteration i runs the LDS kernel if bit i of lds_mask is set (steps 1, 2, 4
// only), else the direct one.
struct DnRecords {
  const float4* A;
  const float4* B;
  const float* ap;
};
bool dn_passes(const FrameRef& F, const Guides& g, const DnParams& P, uint32_t lds_mask, char* scratch, DnRecords& rec,
               std::string& err) {
  hipStream_t s = F.stream;
  const uint32_t W = F.W, H = F.H;
  const size_t np = (size_t)W * H;
  const DnLayout Z(np);
  float4* A[2] = {(float4*)(scratch + Z.a0), (float4*)(scratch + Z.a1)};
  float4* B = (float4*)(scratch + Z.b);
  float* ap = (float*)(scratch + Z.ap);
  k_dn_pack<<<blocks_for(np), kBlock, 0, s>>>(F.acc, F.cnt, g.t, g.normal, g.albedo, g.kind, (uint32_t)np, P.flags,
                                               A[0], B, ap);
  HIP_OK(hipGetLastError());
  const dim3 grid((W + kDnTile - 1) / kDnTile, (H + kDnTile - 1) / kDnTile);
  float sig = P.sigma_c;
  int cur = 0;
  for (uint32_t i = 0; i < P.iterations; i++) {
    const float s2 = sig * sig;
    const bool lds = (lds_mask >> i & 1u) != 0;
    switch (i) {
      case 0: launch_atrous<1>(lds, grid, s, A[cur], B, W, H, s2, P.sigma_z, A[cur ^ 1]); break;
      case 1: launch_atrous<2>(lds, grid, s, A[cur], B, W, H, s2, P.sigma_z, A[cur ^ 1]); break;
      case 2: launch_atrous<4>(lds, grid, s, A[cur], B, W, H, s2, P.sigma_z, A[cur ^ 1]); break;
      case 3: launch_atrous<8>(lds, grid, s, A[cur], B, W, H, s2, P.sigma_z, A[cur ^ 1]); break;
      default: launch_atrous<16>(lds, grid, s, A[cur], B, W, H, s2, P.sigma_z, A[cur ^ 1]); break;
    }
    HIP_OK(hipGetLastError());
    cur ^= 1;
    sig = sig * 0.5f;
  }
  rec = DnRecords{A[cur], B, ap};
  return true;
}

// The filter over device planes: dn_passes, then unpack; the outputs wanted
// are copied to the host and waited for.
bool dn_run(const FrameRef& F, const Guides& g, const DnParams& P, uint32_t lds_mask, char* scratch, const PostOut& O,
            std::string& err, bool dev_out = false) {
  DnRecords R;
  if (!dn_passes(F, g, P, lds_mask, scratch, R, err)) return false;
  const size_t np = (size_t)F.W * F.H;
  const DnLayout Z(np);
  const PostOut dev = {O.rgb3 ? (float*)(scratch + Z.rgb) : nullptr, O.valid ? (uint8_t*)(scratch + Z.valid) : nullptr,
                       O.rgba ? (uint8_t*)(scratch + Z.rgba) : nullptr};
  k_dn_unpack<<<blocks_for(np), kBlock, 0, F.stream>>>(R.A, R.B, R.ap, (uint32_t)np, dev.rgb3, dev.valid, dev.rgba);
  HIP_OK(hipGetLastError());
  return copy_out(F.stream, O, dev, np, err, dev_out);
}

// ---------------------------------------------------------------------------
// Guided upsampling (wpt_upsample.h)
// ---------------------------------------------------------------------------

// The upsampling's coarse stage is the filter with the albedo flag on, whatever
// flags the call's parameters carry.
DnParams coarse_stage(DnParams P) {
  P.flags = kDnAlbedo;
  return P;
}

// k_upsample on F.stream after the passes dn_passes queued there, over their
// records and the fine device planes `hi`; the outputs in up_scratch
// (UpLayout(fine pixels)), copied to the host and waited for.
bool up_run(const FrameRef& F, uint32_t scale, const DnRecords& R, const Guides& hi, float sigma_z, char* up_scratch,
            const PostOut& O, std::string& err) {
  UpParams P;
  P.A.W = F.W; P.A.H = F.H; P.A.s = scale;
  P.A.sigma_z = sigma_z;
  P.A.bg = mk(F.bg[0], F.bg[1], F.bg[2]);
  P.fw = scale * F.W; P.fh = scale * F.H;
  const size_t nf = (size_t)P.fw * P.fh;
  const UpLayout U(nf);
  P.rec.A = R.A;
  P.rec.B = R.B;
  P.t = hi.t; P.normal = hi.normal; P.albedo = hi.albedo; P.kind = hi.kind;
  P.rgb = O.rgb3 ? (float*)(up_scratch + U.rgb) : nullptr;
  P.rgba = O.rgba ? (uint8_t*)(up_scratch + U.rgba) : nullptr;
  P.valid = O.valid ? (uint8_t*)(up_scratch + U.valid) : nullptr;
  const dim3 grid((P.fw + kDnTile - 1) / kDnTile, (P.fh + kDnTile - 1) / kDnTile);
  k_upsample<<<grid, kBlock, 0, F.stream>>>(P);
  HIP_OK(hipGetLastError());
  return copy_out(F.stream, O, PostOut{P.rgb, P.valid, P.rgba}, nf, err);
}

// ---------------------------------------------------------------------------
// Guided sampling (wpt_guided.h)
// ---------------------------------------------------------------------------

// The kernels of sample_map over device planes in a scratch of MapLayout(np):
// needs, their scan, T back to the host, then the deal, which is launched only
// if T is below 2^32.
bool map_run(hipStream_t s, const MapPlanes& in, char* scratch, const MapParams& P, const MapOut& O, bool& invalid,
             std::string& err) {
  const uint32_t np = in.np;
  const MapLayout L(np);
  u64* pre = (u64*)(scratch + L.pre);
  u64* sums = (u64*)(scratch + L.sums);
  uint32_t* count = (uint32_t*)(scratch + L.count);
  const uint32_t n = np + 1;
  k_map_need<<<blocks_for(n), kBlock, 0, s>>>(np, in.cnt, in.len, in.kind, in.member, P.target, P.max_pp, P.flags, pre);
  k_scan64_local<<<L.nb, kBlock, 0, s>>>(pre, n, sums);
  k_scan64_sums<<<1, kBlock, 0, s>>>(sums, L.nb);
  k_scan64_add<<<L.nb, kBlock, 0, s>>>(pre, n, sums);
  HIP_OK(hipGetLastError());
  uint64_t T = 0;
  HIP_OK(hipMemcpyAsync(&T, pre + np, sizeof T, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (O.total) { O.total[0] = T; O.total[1] = 0; }
  if (T >= (1ull << 32)) {
    invalid = true;
    err = "sample_map: the needs sum to 2^32 or more (lower max_per_pixel)";
    return false;
  }
  k_map_deal<<<blocks_for(np), kBlock, 0, s>>>(np, pre, P.budget, count);
  HIP_OK(hipGetLastError());
  if (O.count) HIP_OK(hipMemcpyAsync(O.count, count, 4 * (size_t)np, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (O.total) O.total[1] = map_dealt(P.budget, T);
  return true;
}

}  // namespace

// ===========================================================================
// FramePost
// ===========================================================================

void FramePost::release(Sized by) {
  if (by == Sized::kPartition) {
    d_map_.reset();
    map_ok_ = false;
    return;
  }
  d_dn_.reset();
  d_up_.reset();
  d_hist_[0].reset();
  d_hist_[1].reset();
  d_rp_.reset();
  hist_cur_ = -1;
  rp_merged_ = false;
}

const uint32_t* FramePost::map_counts(uint64_t epoch, size_t np) const {
  if (!(map_ok_ && d_map_ && map_epoch_ == epoch)) return nullptr;
  return (const uint32_t*)(d_map_ + MapLayout(np).count);
}

bool FramePost::denoise(const FrameRef& F, const Guides& g, const DnParams& P, const PostOut& O, std::string& err,
                        bool dev_out) {
  HIP_OK(d_dn_.grow(DnLayout((size_t)F.W * F.H).bytes));
  return dn_run(F, g, P, dn_lds_, d_dn_, O, err, dev_out);
}

bool FramePost::denoise_planes(hipStream_t s, const HostFrame& h, const Guides& hg, const DnParams& P,
                               const PostOut& O, std::string& err) {
  if (!s) { err = "no device"; return false; }
  if (!wanted(O)) return true;
  const size_t np = (size_t)h.W * h.H;
  HookScratch S;
  float4* d_acc = S.d<float4>(np);
  uint32_t* d_cnt = S.d<uint32_t>(np);
  char* scratch = S.d<char>(DnLayout(np).bytes);
  Guides g;
  if (!upload_guides(s, S, hg, np, g, err)) return false;
  if (!S.ok) { err = "hipMalloc failed (denoise_planes)"; return false; }
  std::vector<float4> a4;
  FrameRef F;
  if (!upload_frame(s, h, d_acc, d_cnt, a4, F, err)) return false;
  HIP_OK(hipStreamSynchronize(s));
  return dn_run(F, g, P, dn_lds_, scratch, O, err);
}

// The merged frame and the guide planes stay in d_rp_ for denoise_merged,
// upsample and sample_map; rp_merged_ is down while they are being written.
bool FramePost::reproject(const FrameRef& F, const Guides& g, const RpTest& T, const RpHostOut& O, std::string& err) {
  const bool keep = (T.flags & kRpKeep) != 0;
  const size_t np = (size_t)F.W * F.H;
  const RpMergedLayout ML(np);
  const RpHistLayout HL(np);
  HIP_OK(d_rp_.grow(ML.bytes));
  const int into = hist_cur_ == 0 ? 1 : 0;  // the kept frame not being read
  if (keep) HIP_OK(d_hist_[into].grow(HL.bytes));
  rp_merged_ = false;
  const RpMerged M = ML.at(d_rp_.get());
  RpParams P;
  P.A.W = F.W; P.A.H = F.H;
  P.A.cam = mk(F.cam[0], F.cam[1], F.cam[2]);
  P.A.V = rp_view(F.W, F.H, hist_cam_);
  P.A.cos_min = T.cos_min; P.A.eps_z = T.eps_z; P.A.max_len = T.max_len; P.A.flags = T.flags;
  P.npix = (uint32_t)np;
  P.acc = F.acc;
  P.cnt = F.cnt;
  P.dir = g.dir; P.t = g.t; P.id = g.id; P.normal = g.normal; P.kind = g.kind;
  P.hist = hist_cur_ >= 0 ? HL.at(d_hist_[hist_cur_].get()) : kNoHist;
  P.acc_out = M.acc; P.cnt_out = M.cnt; P.len_out = M.len;
  P.keep = keep ? HL.at(d_hist_[into].get()) : kNoHist;
  hipStream_t s = F.stream;
  k_reproject<<<blocks_for(np), kBlock, 0, s>>>(P);
  HIP_OK(hipGetLastError());
  // the guides of this call, out of first_hit's buffer before its next user
  HIP_OK(hipMemcpyAsync(M.t, g.t, 4 * np, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(M.normal, g.normal, 12 * np, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(M.albedo, g.albedo, 12 * np, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(M.kind, g.kind, np, hipMemcpyDeviceToDevice, s));
  if (O.cnt) HIP_OK(hipMemcpyAsync(O.cnt, M.cnt, 4 * np, hipMemcpyDeviceToHost, s));
  if (O.len) HIP_OK(hipMemcpyAsync(O.len, M.len, 4 * np, hipMemcpyDeviceToHost, s));
  HIP_OK(download_rgb3(s, M.acc, np, O.acc3));
  rp_merged_ = true;
  rp_epoch_ = F.epoch;
  if (keep) {
    hist_cur_ = into;
    hist_epoch_ = F.epoch;
    memcpy(hist_cam_, F.cam, sizeof hist_cam_);
  }
  return true;
}

// The history's planes are packed on the host with rp_pack, the function a
// keeping k_reproject packs them with.
bool FramePost::reproject_planes(hipStream_t s, const HostFrame& h, const Guides& hg, const HostFrame& hist,
                                 const Guides& histg, const RpTest& T, const RpHostOut& O, std::string& err) {
  if (!s) { err = "no device"; return false; }
  if (!O.acc3 && !O.cnt && !O.len) return true;
  const size_t np = (size_t)h.W * h.H;
  const RpHistLayout HL(np);
  HookScratch S;
  float4* d_acc = S.d<float4>(2 * np);  // in, then out
  uint32_t* d_cnt = S.d<uint32_t>(3 * np);  // in, out, len
  char* d_h = S.d<char>(HL.bytes);
  Guides g;
  if (!upload_guides(s, S, hg, np, g, err)) return false;
  if (!S.ok) { err = "hipMalloc failed (reproject_planes)"; return false; }
  std::vector<float4> a4;
  std::vector<char> hb(HL.bytes, 0);
  const RpHist hh = HL.at(hb.data());
  for (size_t i = 0; i < np; i++) {
    const RpKept k = rp_pack(mk(hist.acc3[3 * i], hist.acc3[3 * i + 1], hist.acc3[3 * i + 2]), hist.cnt[i]);
    hh.k[i] = (uint32_t)histg.kind[i] | (k.valid ? 0x100u : 0u);
    hh.r0[i] = make_float4(k.c.x, k.c.y, k.c.z, u2f(hist.cnt[i]));
    hh.r1[i] = make_float4(histg.normal[3 * i], histg.normal[3 * i + 1], histg.normal[3 * i + 2], histg.t[i]);
    hh.id[i] = histg.id[i];
  }
  FrameRef F;
  if (!upload_frame(s, h, d_acc, d_cnt, a4, F, err)) return false;
  HIP_OK(hipMemcpyAsync(d_h, hb.data(), HL.bytes, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));
  RpParams P;
  P.A.W = h.W; P.A.H = h.H;
  P.A.cam = mk(h.cam[0], h.cam[1], h.cam[2]);
  P.A.V = rp_view(h.W, h.H, hist.cam);
  P.A.cos_min = T.cos_min; P.A.eps_z = T.eps_z; P.A.max_len = T.max_len; P.A.flags = T.flags;
  P.npix = (uint32_t)np;
  P.acc = d_acc; P.cnt = d_cnt;
  P.dir = g.dir; P.t = g.t; P.id = g.id; P.normal = g.normal; P.kind = g.kind;
  P.hist = HL.at(d_h);
  P.acc_out = d_acc + np; P.cnt_out = d_cnt + np; P.len_out = d_cnt + 2 * np;
  P.keep = kNoHist;
  k_reproject<<<blocks_for(np), kBlock, 0, s>>>(P);
  HIP_OK(hipGetLastError());
  if (O.cnt) HIP_OK(hipMemcpyAsync(O.cnt, P.cnt_out, 4 * np, hipMemcpyDeviceToHost, s));
  if (O.len) HIP_OK(hipMemcpyAsync(O.len, P.len_out, 4 * np, hipMemcpyDeviceToHost, s));
  HIP_OK(download_rgb3(s, P.acc_out, np, O.acc3));
  return true;
}

bool FramePost::denoise_merged(const FrameRef& F, const DnParams& P, const PostOut& O, std::string& err) {
  if (!rp_merged_ || !d_rp_) { err = "no merged frame"; return false; }
  if (!wanted(O)) return true;
  const size_t np = (size_t)F.W * F.H;
  HIP_OK(d_dn_.grow(DnLayout(np).bytes));
  const RpMerged M = RpMergedLayout(np).at(d_rp_.get());
  FrameRef merged = F;
  merged.acc = M.acc;
  merged.cnt = M.cnt;
  return dn_run(merged, M.guides(), P, dn_lds_, d_dn_, O, err);
}

// Everything stays on the device; the history and the sample map are only read.
bool FramePost::upsample(const FrameRef& F, const Guides* lo, uint32_t scale, const Guides& hi, const DnParams& P,
                         const PostOut& O, std::string& err) {
  const size_t np = (size_t)F.W * F.H, nf = (size_t)scale * F.W * ((size_t)scale * F.H);
  HIP_OK(d_dn_.grow(DnLayout(np).bytes));
  HIP_OK(d_up_.grow(UpLayout(nf).bytes));
  FrameRef src = F;
  Guides g;
  if (lo) {
    g = *lo;
  } else {
    const RpMerged M = RpMergedLayout(np).at(d_rp_.get());
    src.acc = M.acc;
    src.cnt = M.cnt;
    g = M.guides();
  }
  DnRecords R;
  if (!dn_passes(src, g, coarse_stage(P), dn_lds_, d_dn_, R, err)) return false;
  return up_run(F, scale, R, hi, P.sigma_z, d_up_, O, err);
}

bool FramePost::upsample_planes(hipStream_t s, const HostFrame& h, const Guides& hlo, uint32_t scale,
                                const Guides& hhi, const DnParams& P, const PostOut& O, std::string& err) {
  if (!s) { err = "no device"; return false; }
  if (!wanted(O)) return true;
  const size_t np = (size_t)h.W * h.H, nf = (size_t)scale * h.W * ((size_t)scale * h.H);
  HookScratch S;
  float4* d_acc = S.d<float4>(np);
  uint32_t* d_cnt = S.d<uint32_t>(np);
  char* dn_scratch = S.d<char>(DnLayout(np).bytes);
  char* up_scratch = S.d<char>(UpLayout(nf).bytes);
  Guides lo, hi;
  if (!upload_guides(s, S, hlo, np, lo, err) || !upload_guides(s, S, hhi, nf, hi, err)) return false;
  if (!S.ok) { err = "hipMalloc failed (upsample_planes)"; return false; }
  std::vector<float4> a4;
  FrameRef F;
  if (!upload_frame(s, h, d_acc, d_cnt, a4, F, err)) return false;
  HIP_OK(hipStreamSynchronize(s));
  DnRecords R;
  if (!dn_passes(F, lo, coarse_stage(P), dn_lds_, dn_scratch, R, err)) return false;
  return up_run(F, scale, R, hi, P.sigma_z, up_scratch, O, err);
}

// The len plane is the one the last reproject of this accumulation left in
// d_rp_ (else 0 everywhere). map_ok_ is down while the map is being written.
bool FramePost::sample_map(const FrameRef& F, const uint8_t* kind, const std::vector<uint8_t>* member,
                           const MapParams& P, const MapOut& O, bool& invalid, std::string& err) {
  const size_t np = (size_t)F.W * F.H;
  const MapLayout L(np);
  HIP_OK(d_map_.grow(L.bytes));
  map_ok_ = false;
  char* m = d_map_;
  MapPlanes in = {(uint32_t)np, F.cnt, nullptr, kind, nullptr};
  if (member) {
    HIP_OK(hipMemcpyAsync(m + L.member, member->data(), np, hipMemcpyHostToDevice, F.stream));
    HIP_OK(hipStreamSynchronize(F.stream));
    in.member = (const uint8_t*)(m + L.member);
  }
  if (rp_merged_ && d_rp_ && rp_epoch_ == F.epoch) in.len = RpMergedLayout(np).at(d_rp_.get()).len;
  if (!map_run(F.stream, in, m, P, O, invalid, err)) return false;
  map_ok_ = true;
  map_epoch_ = F.epoch;
  return true;
}

bool FramePost::sample_map_planes(hipStream_t s, const MapPlanes& h, const MapParams& P, const MapOut& O,
                                  bool& invalid, std::string& err) {
  invalid = false;
  if (!s) { err = "no device"; return false; }
  const size_t np = h.np;
  HookScratch S;
  uint32_t* d_cnt = S.d<uint32_t>(2 * np);  // cnt, len
  uint8_t* d_km = S.d<uint8_t>(2 * np);     // kind, member
  char* d_s = S.d<char>(MapLayout(np).bytes);
  if (!S.ok) { err = "hipMalloc failed (sample_map_planes)"; return false; }
  HIP_OK(hipMemcpyAsync(d_cnt, h.cnt, 4 * np, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(d_cnt + np, h.len, 4 * np, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(d_km, h.kind, np, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(d_km + np, h.member, np, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));
  return map_run(s, MapPlanes{h.np, d_cnt, d_cnt + np, d_km, d_km + np}, d_s, P, O, invalid, err);
}

}  // namespace wpt
