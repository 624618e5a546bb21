// wpt_upsample.h — guided upsampling of a W x H frame to s W x s H
// (wpt_upsample, wpt_upsample_planes, wpt_upsample_host; include/wpt.h; the
// definition to the operation: DESIGN.md §2).
//
// Joint bilateral upsampling (Kopf et al. 2007) with albedo demodulation: the
// geometry of the fine frame (edges, emitters, albedo) comes from first-hit
// planes made at the fine viewport, the slowly varying irradiance from the
// coarse frame. The reference knows diffuse and emissive materials only, so a
// directly seen emitter and a miss are known exactly at the fine viewport and
// only diffuse pixels are interpolated. The coarse stage is the filter's own
// (wpt_denoise.h: dn_pack with the albedo flag on, then the a-trous passes);
// a fine diffuse pixel then takes the four coarse pixels around it with
// bilinear x normal x depth weights (the filter's d^32 and 1 / (1 + r^2)), a
// 4 x 4 block with flat spatial weights if none of the four passes, and
// multiplies its own albedo back. Only + - * /, comparisons and max, each one
// rounded f32 operation in the order written, nothing contracted (FPFLAGS).
//
// Arithmetic contract: the filter's. The host restatement (upsample_host) and
// the kernel agree on every bit of every output while |acc / cnt| <= 2^100.
//
// Two parts, like wpt_denoise.h, after which it is included inside namespace
// wpt: plain C++ for host and device (the tap positions, one tap, one fine
// pixel, the host restatement), then the kernel (WPT_UPSAMPLE_KERNELS,
// wpt_post.hip), which calls the same functions.
//
// k_upsample: one lane per fine pixel, 16 x 16 fine tiles (k_dn_atrous's
// geometry). A lane reads its fine guides (t, normal, albedo, kind: 29 B), and
// a diffuse one its taps straight from global memory out of the filter's
// records: B = {n, kind | valid << 8} first (128 bit), A = {c', t} only if B
// passes. A 16 x 16 tile touches (16 / s + 2)^2 coarse records, each reused by
// about 4 s^2 lanes of the tile: the reuse is left to L1 / L2.
#pragma once

constexpr uint32_t kUpMerged = 1u;       // WPT_UPSAMPLE_MERGED
constexpr uint32_t kUpMaxScale = 4;
constexpr uint32_t kUpTapWord = 0x101u;  // B's word of a tap: diffuse, with samples and a finite value

// Fine coordinate X of a frame s times as wide: the coarse pixel i0 left of
// (above) its centre, which may be -1, and the fraction f towards i0 + 1.
// a = 2X + 1 - s, i0 = floor(a / 2s), m = a - 2s i0, f = m / 2s; with
// X = s q + r this is a = 2s q + e, e = 2r + 1 - s in (-s, s).
WPT_HD void up_axis(uint32_t X, uint32_t s, long long& i0, float& f) {
  const uint32_t q = X / s, r = X % s;
  const int e = 2 * (int)r + 1 - (int)s;
  i0 = e >= 0 ? (long long)q : (long long)q - 1;
  const int m = e >= 0 ? e : e + 2 * (int)s;
  f = (float)m / (float)(2u * s);
}

// A coarse pixel that may be a tap: the filtered irradiance c', normal, depth.
struct UpTap {
  V3 c, n;
  float t;
};
struct UpArgs {
  uint32_t W, H, s;  // the coarse viewport and the scale
  float sigma_z;
  V3 bg;             // the scene's background
};
struct UpOut {
  V3 o;
  uint8_t valid;  // 0 nothing passed, 1 exact or the four taps, 2 the 4 x 4 block
};

// One tap of fine pixel (N, T): wb the spatial weight, zden = sigma_z * T.
// fetch(q, tap) gives coarse pixel q, or false unless it is diffuse, has
// samples and a finite value.
template <class Fetch>
WPT_HD void up_tap(DnTapSum& S, const UpArgs& A, const Fetch& fetch, long long qx, long long qy, float wb, V3 N, float T,
                   float zden) {
  if (qx < 0 || qy < 0 || qx >= (long long)A.W || qy >= (long long)A.H) return;
  UpTap q;
  if (!fetch((size_t)qy * A.W + (size_t)qx, q)) return;
  float d = fmaxf((N.x * q.n.x + N.y * q.n.y) + N.z * q.n.z, 0.0f);
  d = d * d;
  d = d * d;
  d = d * d;
  d = d * d;
  d = d * d;  // d^32, dn_weight's
  const float r = fabsf(T - q.t) / zden;
  const float w = (wb * d) * (1.0f / (1.0f + r * r));
  if (!(w > 0.0f)) return;  // also the NaN of 0 / 0
  dn_add(S, w, q.c);
}

// Fine pixel (X, Y) with guides T, N, Al, K.
template <class Fetch>
WPT_HD UpOut up_pixel(const UpArgs& A, const Fetch& fetch, uint32_t X, uint32_t Y, float T, V3 N, V3 Al, uint32_t K) {
  UpOut o;
  o.valid = 1;
  if (K == 0u) { o.o = A.bg; return o; }
  if (K != 1u) { o.o = Al; return o; }  // an emitter: its intensity
  long long x0, y0;
  float fx, fy;
  up_axis(X, A.s, x0, fx);
  up_axis(Y, A.s, y0, fy);
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float zden = A.sigma_z * T;
  DnTapSum S{mk(0.0f, 0.0f, 0.0f), 0.0f};
  up_tap(S, A, fetch, x0, y0, gx * gy, N, T, zden);
  up_tap(S, A, fetch, x0 + 1, y0, fx * gy, N, T, zden);
  up_tap(S, A, fetch, x0, y0 + 1, gx * fy, N, T, zden);
  up_tap(S, A, fetch, x0 + 1, y0 + 1, fx * fy, N, T, zden);
  if (!(S.sw > 0.0f)) {
    o.valid = 2;
    for (int dy = -1; dy <= 2; dy++)
      for (int dx = -1; dx <= 2; dx++) up_tap(S, A, fetch, x0 + dx, y0 + dy, 1.0f, N, T, zden);
  }
  if (!(S.sw > 0.0f)) {
    o.o = mk(0.0f, 0.0f, 0.0f);
    o.valid = 0;
    return o;
  }
  const V3 e = mk(S.a.x / S.sw, S.a.y / S.sw, S.a.z / S.sw);
  const V3 ap = mk(Al.x > 0.0f ? Al.x : 1.0f, Al.y > 0.0f ? Al.y : 1.0f, Al.z > 0.0f ? Al.z : 1.0f);
  o.o = mk(e.x * ap.x, e.y * ap.y, e.z * ap.z);
  return o;
}

// The restatement on the host: the filter's pack and passes, then pixel by pixel.
struct UpPlaneFetch {
  const DnHostFrame* F;
  const float* t;
  const float* n;
  const uint8_t* kind;
  bool operator()(size_t q, UpTap& o) const {
    if (!F->ok[q] || kind[q] != 1u) return false;
    o.c = F->c[q];
    o.n = mk(n[3 * q], n[3 * q + 1], n[3 * q + 2]);
    o.t = t[q];
    return true;
  }
};

inline void upsample_host(uint32_t W, uint32_t H, uint32_t scale, const float* acc3, const uint32_t* cnt, const float* t,
                          const float* normal3, const float* albedo3, const uint8_t* kind, const float* hi_t,
                          const float* hi_normal3, const float* hi_albedo3, const uint8_t* hi_kind,
                          const float* background3, uint32_t iterations, float sigma_c, float sigma_z, float* rgb3,
                          uint8_t* valid, uint8_t* rgba) {
  DnHostFrame F;
  dn_host_passes(W, H, acc3, cnt, t, normal3, albedo3, kind, iterations, sigma_c, sigma_z, kDnAlbedo, F);
  UpArgs A;
  A.W = W; A.H = H; A.s = scale;
  A.sigma_z = sigma_z;
  A.bg = mk(background3[0], background3[1], background3[2]);
  const UpPlaneFetch fetch{&F, t, normal3, kind};
  const uint32_t fw = scale * W, fh = scale * H;
  for (uint32_t Y = 0; Y < fh; Y++)
    for (uint32_t X = 0; X < fw; X++) {
      const size_t i = (size_t)Y * fw + X, j = 3 * i;
      const UpOut o = up_pixel(A, fetch, X, Y, hi_t[i], mk(hi_normal3[j], hi_normal3[j + 1], hi_normal3[j + 2]),
                               mk(hi_albedo3[j], hi_albedo3[j + 1], hi_albedo3[j + 2]), hi_kind[i]);
      if (rgb3) { rgb3[j] = o.o.x; rgb3[j + 1] = o.o.y; rgb3[j + 2] = o.o.z; }
      if (valid) valid[i] = o.valid;
      if (rgba) {
        rgba[4 * i] = dn_quant(o.o.x);
        rgba[4 * i + 1] = dn_quant(o.o.y);
        rgba[4 * i + 2] = dn_quant(o.o.z);
        rgba[4 * i + 3] = 255;
      }
    }
}

#if defined(WPT_UPSAMPLE_KERNELS)

struct UpRecFetch {
  const float4* A;  // {c', t}
  const float4* B;  // {n, kind | valid << 8}
  __device__ __forceinline__ bool operator()(size_t q, UpTap& o) const {
    const float4 b = B[q];
    if (__float_as_uint(b.w) != kUpTapWord) return false;
    const float4 a = A[q];
    o.c = mk(a.x, a.y, a.z);
    o.n = mk(b.x, b.y, b.z);
    o.t = a.w;
    return true;
  }
};

struct UpParams {
  UpArgs A;
  uint32_t fw, fh;  // the fine viewport: s W x s H
  UpRecFetch rec;   // the coarse stage's records
  const float* t;   // the fine guides, k_first_hit's planes
  const float* normal;
  const float* albedo;
  const uint8_t* kind;
  float* rgb;  // a null output is not written
  uint8_t* valid;
  uint8_t* rgba;
};

__global__ void __launch_bounds__(kBlock) k_upsample(const UpParams P) {
  const uint32_t X = blockIdx.x * kDnTile + threadIdx.x % kDnTile, Y = blockIdx.y * kDnTile + threadIdx.x / kDnTile;
  if (X >= P.fw || Y >= P.fh) return;
  const size_t i = (size_t)Y * P.fw + X, j = 3 * i;
  const UpOut o = up_pixel(P.A, P.rec, X, Y, P.t[i], mk(P.normal[j], P.normal[j + 1], P.normal[j + 2]),
                           mk(P.albedo[j], P.albedo[j + 1], P.albedo[j + 2]), P.kind[i]);
  if (P.rgb) st3(P.rgb + j, o.o);
  if (P.valid) P.valid[i] = o.valid;
  if (P.rgba) reinterpret_cast<uchar4*>(P.rgba)[i] = make_uchar4(dn_quant(o.o.x), dn_quant(o.o.y), dn_quant(o.o.z), 255);
}

#endif  // WPT_UPSAMPLE_KERNELS
