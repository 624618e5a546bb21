// wpt_reproject.h — reverse reprojection of a kept history frame into the
// current camera (wpt_reproject, wpt_reproject_planes, wpt_reproject_host;
// include/wpt.h; the definition to the operation: DESIGN.md §2).
//
// The reference resets its accumulation at every camera move
// (wasm_interface.rs:239-248); its materials are diffuse and emissive only, so
// the radiance a surface point gathered under the previous camera holds under
// the new one. Per current pixel: the first hit's world point is projected into
// the previous view (the inverse of primary_dir's two rotations), one or four
// history pixels around it are tested by kind, shape id (on request), normal
// and depth, and their weighted mean enters the current sums with the smallest
// sample count among them, capped by max_len. Only + - * /, sqrt, floor,
// comparisons and min, each one rounded f32 operation in the order written,
// nothing contracted (FPFLAGS).
//
// Arithmetic contract: the host restatement (reproject_host below) and
// k_reproject agree on every bit of every output while every finite history
// mean and current sum is at most 2^100 in magnitude.
//
// Two parts. The first is plain C++ for host and device: the projection, the
// test and the sum of one tap, the merge, the pack of a kept pixel, and the
// host restatement that calls them on planes. The second (WPT_REPROJECT_KERNELS,
// wpt_post.hip) holds k_reproject, which calls the same functions on the
// history's records. Included inside namespace wpt, after wpt_denoise.h.
//
// A kept pixel is 40 bytes in four planes, so that a tap is one word and two
// 128-bit loads:
//   K  u32     kind | valid << 8; valid: it has samples and a finite mean
//   R0 float4  {mean.xyz, count as bits}
//   R1 float4  {normal.xyz, t}
//   ID i32     the shape id, read only under WPT_REPROJECT_SAME_SHAPE
// K settles "has samples, a finite mean and my kind" in one compare before
// either record is fetched (as k_dn_atrous's direct variant does with B). The
// history is not staged in LDS: which window a block gathers depends on the
// data, and under a rigid camera motion neighbouring lanes' taps are
// neighbours, so the reuse is L2's.
#pragma once

constexpr uint32_t kRpKeep = 1u, kRpNearest = 2u, kRpSameShape = 4u;  // WPT_REPROJECT_*
constexpr uint32_t kRpMaxLen = 1u << 24;

// The previous camera: its position, cos / sin of rot_x and rot_y (make_view:
// the kernel never evaluates a sine) and the viewport as floats.
struct RpView {
  V3 pcam;
  float cx, sx, cy, sy, fw, fh, ar;
};
inline RpView rp_view(uint32_t W, uint32_t H, const float* pcam5) {
  const View v = make_view(W, H, pcam5[3], pcam5[4]);
  RpView r;
  r.pcam = mk(pcam5[0], pcam5[1], pcam5[2]);
  r.cx = v.cx; r.sx = v.sx; r.cy = v.cy; r.sy = v.sy;
  r.fw = (float)W; r.fh = (float)H; r.ar = v.ar;
  return r;
}

// The world point of a first hit in the previous view: (u, v) with pixel
// centres at integers, te its distance from the previous camera. False if the
// point is behind that camera or outside (-1, fw) x (-1, fh); NaN fails too,
// so that every float-to-int conversion after it is defined.
WPT_HD bool rp_project(const RpView& V, V3 cam, V3 dir, float t, float& u, float& v, float& te) {
  const V3 P = mk(cam.x + t * dir.x, cam.y + t * dir.y, cam.z + t * dir.z);
  const V3 d = sub(P, V.pcam);
  te = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
  const V3 v1 = mk(V.cy * d.x - V.sy * d.z, d.y, V.sy * d.x + V.cy * d.z);              // rot_y back
  const V3 v2 = mk(v1.x, V.cx * v1.y + V.sx * v1.z, (-V.sx) * v1.y + V.cx * v1.z);      // rot_x back
  if (!(v2.z > 0.0f)) return false;
  const float k = 0.8f / v2.z;
  u = ((v2.x * k) / V.ar + 0.5f) * V.fw - 0.5f;
  v = (0.5f - v2.y * k) * V.fh - 0.5f;
  return u > -1.0f && u < V.fw && v > -1.0f && v < V.fh;
}

// A kept pixel: the mean and whether a tap may use it.
struct RpKept {
  V3 c;
  bool valid;
};
WPT_HD RpKept rp_pack(V3 acc, uint32_t cnt) {
  RpKept k;
  const float fc = (float)cnt;
  k.c = mk(acc.x / fc, acc.y / fc, acc.z / fc);
  k.valid = cnt > 0 && dn_finite(k.c.x) && dn_finite(k.c.y) && dn_finite(k.c.z);
  return k;
}

// A tap that has samples, a finite mean c, the centre's kind and, where asked
// for, its shape id.
struct RpTap {
  V3 c, n;
  uint32_t cnt;
  float t;
};
struct RpSum {
  V3 s;
  float sw;
  uint32_t lmin;
};
// the tests on normal, depth and weight, then the sums
WPT_HD void rp_add(RpSum& S, float w, const RpTap& q, V3 n_p, float te, float cos_min, float eps_z) {
  if (!((n_p.x * q.n.x + n_p.y * q.n.y) + n_p.z * q.n.z >= cos_min)) return;
  if (!(fabsf(q.t - te) <= eps_z * te)) return;
  if (!(w > 0.0f)) return;
  S.s = mk(S.s.x + w * q.c.x, S.s.y + w * q.c.y, S.s.z + w * q.c.z);
  S.sw = S.sw + w;
  S.lmin = q.cnt < S.lmin ? q.cnt : S.lmin;
}

struct RpOut {
  V3 acc;
  uint32_t cnt, len;
};
struct RpArgs {
  uint32_t W, H;
  V3 cam;
  RpView V;
  float cos_min, eps_z;
  uint32_t max_len, flags;
};

template <class Fetch>
WPT_HD void rp_tap(RpSum& S, const RpArgs& A, const Fetch& fetch, long long qx, long long qy, float w, uint32_t kind,
                   int32_t id, V3 n_p, float te) {
  if (qx < 0 || qy < 0 || qx >= (long long)A.W || qy >= (long long)A.H) return;
  RpTap q;
  if (!fetch((size_t)qy * A.W + (size_t)qx, kind, id, q)) return;
  rp_add(S, w, q, n_p, te, A.cos_min, A.eps_z);
}

// One current pixel. fetch(q, kind, id, tap) gives history pixel q, or false if
// it has no samples, no finite mean, another kind or (SAME_SHAPE) another id.
template <class Fetch>
WPT_HD RpOut rp_pixel(const RpArgs& A, const Fetch& fetch, V3 acc, uint32_t cnt, V3 dir, float t, int32_t id, V3 n_p,
                      uint32_t kind) {
  RpOut o;
  o.acc = acc; o.cnt = cnt; o.len = 0;
  if (kind == 0 || !dn_finite(acc.x) || !dn_finite(acc.y) || !dn_finite(acc.z)) return o;
  float u, v, te;
  if (!rp_project(A.V, A.cam, dir, t, u, v, te)) return o;
  RpSum S;
  S.s = mk(0.0f, 0.0f, 0.0f); S.sw = 0.0f; S.lmin = 0xFFFFFFFFu;
  if (A.flags & kRpNearest) {
    rp_tap(S, A, fetch, (long long)floorf(u + 0.5f), (long long)floorf(v + 0.5f), 1.0f, kind, id, n_p, te);
  } else {
    const float x0 = floorf(u), y0 = floorf(v);
    const float fx = u - x0, fy = v - y0, gx = 1.0f - fx, gy = 1.0f - fy;
    const long long ix = (long long)x0, iy = (long long)y0;
    rp_tap(S, A, fetch, ix, iy, gx * gy, kind, id, n_p, te);
    rp_tap(S, A, fetch, ix + 1, iy, fx * gy, kind, id, n_p, te);
    rp_tap(S, A, fetch, ix, iy + 1, gx * fy, kind, id, n_p, te);
    rp_tap(S, A, fetch, ix + 1, iy + 1, fx * fy, kind, id, n_p, te);
  }
  if (!(S.sw > 0.0f)) return o;
  const V3 h = mk(S.s.x / S.sw, S.s.y / S.sw, S.s.z / S.sw);
  const uint32_t room = 0xFFFFFFFFu - cnt;
  uint32_t L = S.lmin < A.max_len ? S.lmin : A.max_len;
  L = L < room ? L : room;
  const float fl = (float)L;
  o.acc = mk(acc.x + h.x * fl, acc.y + h.y * fl, acc.z + h.z * fl);
  o.cnt = cnt + L;
  o.len = L;
  return o;
}

// The restatement on the host: the same functions on the history's planes.
struct RpPlaneFetch {
  const float* hacc;
  const uint32_t* hcnt;
  const float* ht;
  const int32_t* hid;
  const float* hn;
  const uint8_t* hkind;
  bool same;
  bool operator()(size_t q, uint32_t kind, int32_t id, RpTap& o) const {
    if (hkind[q] != kind) return false;
    if (same && hid[q] != id) return false;
    const RpKept k = rp_pack(mk(hacc[3 * q], hacc[3 * q + 1], hacc[3 * q + 2]), hcnt[q]);
    if (!k.valid) return false;
    o.c = k.c;
    o.n = mk(hn[3 * q], hn[3 * q + 1], hn[3 * q + 2]);
    o.cnt = hcnt[q];
    o.t = ht[q];
    return true;
  }
};

inline void reproject_host(uint32_t W, uint32_t H, const float* cam3, const float* acc3, const uint32_t* cnt,
                           const float* dir3, const float* t, const int32_t* id, const float* normal3,
                           const uint8_t* kind, const float* prev_cam5, const float* h_acc3, const uint32_t* h_cnt,
                           const float* h_t, const int32_t* h_id, const float* h_normal3, const uint8_t* h_kind,
                           float cos_min, float eps_z, uint32_t max_len, uint32_t flags, float* acc3_out,
                           uint32_t* cnt_out, uint32_t* len_out) {
  RpArgs A;
  A.W = W; A.H = H;
  A.cam = mk(cam3[0], cam3[1], cam3[2]);
  A.V = rp_view(W, H, prev_cam5);
  A.cos_min = cos_min; A.eps_z = eps_z; A.max_len = max_len; A.flags = flags;
  const RpPlaneFetch fetch{h_acc3, h_cnt, h_t, h_id, h_normal3, h_kind, (flags & kRpSameShape) != 0};
  const size_t np = (size_t)W * H;
  for (size_t i = 0; i < np; i++) {
    const size_t j = 3 * i;
    const RpOut o = rp_pixel(A, fetch, mk(acc3[j], acc3[j + 1], acc3[j + 2]), cnt[i],
                             mk(dir3[j], dir3[j + 1], dir3[j + 2]), t[i], id[i],
                             mk(normal3[j], normal3[j + 1], normal3[j + 2]), kind[i]);
    if (acc3_out) { acc3_out[j] = o.acc.x; acc3_out[j + 1] = o.acc.y; acc3_out[j + 2] = o.acc.z; }
    if (cnt_out) cnt_out[i] = o.cnt;
    if (len_out) len_out[i] = o.len;
  }
}

#if defined(WPT_REPROJECT_KERNELS)

// The planes of a kept frame of np pixels (see the header comment)
struct RpHist {
  uint32_t* k;
  float4* r0;
  float4* r1;
  int32_t* id;
};

struct RpRecFetch {
  RpHist h;
  bool same;
  __device__ __forceinline__ bool operator()(size_t q, uint32_t kind, int32_t id, RpTap& o) const {
    if (h.k[q] != (kind | 0x100u)) return false;
    if (same && h.id[q] != id) return false;
    const float4 a = h.r0[q], b = h.r1[q];
    o.c = mk(a.x, a.y, a.z);
    o.cnt = __float_as_uint(a.w);
    o.n = mk(b.x, b.y, b.z);
    o.t = b.w;
    return true;
  }
};

struct RpParams {
  RpArgs A;
  uint32_t npix;
  // the current frame (acc: float4 sums) and k_first_hit's planes; id may be
  // null when neither SAME_SHAPE nor keep needs it
  const float4* acc;
  const uint32_t* cnt;
  const float* dir;
  const float* t;
  const int32_t* id;
  const float* normal;
  const uint8_t* kind;
  RpHist hist;   // hist.k null: no history, every pixel passes through
  float4* acc_out;
  uint32_t* cnt_out;
  uint32_t* len_out;
  RpHist keep;   // keep.k null: the merged frame is not kept
};

__device__ __forceinline__ V3 rp_ld3(const float* p) { return mk(p[0], p[1], p[2]); }

// One lane per pixel: the merged frame, and on request its kept records.
__global__ void __launch_bounds__(kBlock) k_reproject(const RpParams P) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= P.npix) return;
  const float4 a = P.acc[i];
  const size_t j = 3 * (size_t)i;
  const V3 n = rp_ld3(P.normal + j);
  const float t = P.t[i];
  const uint32_t kind = P.kind[i];
  const int32_t id = P.id ? P.id[i] : -1;
  RpOut o;
  o.acc = mk(a.x, a.y, a.z); o.cnt = P.cnt[i]; o.len = 0;
  if (P.hist.k) {
    const RpRecFetch fetch{P.hist, (P.A.flags & kRpSameShape) != 0};
    o = rp_pixel(P.A, fetch, o.acc, o.cnt, rp_ld3(P.dir + j), t, id, n, kind);
  }
  P.acc_out[i] = make_float4(o.acc.x, o.acc.y, o.acc.z, a.w);
  P.cnt_out[i] = o.cnt;
  P.len_out[i] = o.len;
  if (P.keep.k) {
    const RpKept k = rp_pack(o.acc, o.cnt);
    P.keep.k[i] = kind | (k.valid ? 0x100u : 0u);
    P.keep.r0[i] = make_float4(k.c.x, k.c.y, k.c.z, __uint_as_float(o.cnt));
    P.keep.r1[i] = make_float4(n.x, n.y, n.z, t);
    P.keep.id[i] = id;
  }
}

#endif  // WPT_REPROJECT_KERNELS
