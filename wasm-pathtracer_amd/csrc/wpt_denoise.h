// wpt_denoise.h — edge-avoiding a-trous filter on the first-hit planes
// (wpt_denoise, wpt_denoise_planes, wpt_denoise_host; include/wpt.h; the
// definition to the operation: DESIGN.md §2).
//
// The filter of Dammertz et al. 2010 over the reference's 5 x 5 GAUSS5 stencil
// (render_target.rs:21-27, the B3-spline kernel), guided by the planes
// k_first_hit makes (depth, normal, albedo, kind), with rational weights
// 1 / (1 + x) in place of exponentials: only + - * /, comparisons and max, each
// one rounded f32 operation in the order written, nothing contracted (FPFLAGS).
//
// Arithmetic contract: the host restatement (denoise_host below) and the
// kernels agree on every bit of every output while |acc / cnt| <= 2^100 in
// every component. Beyond that range a sum can overflow and produce a NaN
// (inf - inf, inf / inf) whose payload differs between x86 and gfx950.
//
// Two parts. The first is plain C++ for host and device: the pack, the weight
// of one tap, the quantisation, and the host restatement that calls them. The
// second (WPT_DENOISE_KERNELS, wpt_post.hip) holds the kernels, which call
// the same functions. Included inside namespace wpt.
//
// Kernels, one lane per pixel:
//  k_dn_pack    acc / cnt and the guides -> two float4 records per pixel:
//               A = {c.xyz, t} (ping-ponged between two planes), B = {n.xyz,
//               kind | valid << 8 as bits} (read-only), and a' (3 f32).
//  k_dn_atrous  one iteration. 16 x 16 pixel tiles, 256 lanes (k_mse_tiled's
//               geometry). LDS variant (steps 1, 2, 4): the block stages its
//               tile plus the 2 * STEP halo of A and B, (16 + 4 * STEP)^2
//               records of each, and every tap is two ds_read_b128. Rows are
//               kDnPitch = 32 records (512 B) apart whatever the tile's side:
//               ds_read_b128 banks per 16-lane group, each group being eight
//               lanes of one tile row and eight of the next covering x = 0..15
//               once, so with a pitch that is a multiple of the 256 B bank row
//               the 16 records of a group fall on 16 different slots (a pitch
//               of 20 or 24 records would make every read 2-way). The largest
//               tile is 32 x 32: 32 KB. Direct variant (every step): taps are
//               two 128-bit global loads (B first; A only for a tap that is
//               not skipped by B), the reuse being left to L2.
//  k_dn_unpack  remodulates with a' and writes rgb, valid and RGBA8.
#pragma once

constexpr uint32_t kDnAlbedo = 1u;  // WPT_DENOISE_ALBEDO
constexpr uint32_t kDnMaxIter = 5;

WPT_HD bool dn_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

// GAUSS5[vy * 5 + vx] (render_target.rs:21-27), as written there
WPT_HD float dn_gauss(int vy, int vx) {
  const float g[3] = {1.0f, 4.0f, 6.0f};
  const float gy = g[vy < 3 ? vy : 4 - vy], gx = g[vx < 3 ? vx : 4 - vx];
  return gy * gx;  // exact: small integers
}

// Pack: the mean, demodulated by the albedo of a diffuse hit when asked for.
struct DnPix {
  V3 c, a;
  bool valid;
};
WPT_HD DnPix dn_pack(V3 acc, uint32_t cnt, V3 albedo, uint32_t kind, uint32_t flags) {
  DnPix p;
  const float fc = (float)cnt;
  const V3 m = mk(acc.x / fc, acc.y / fc, acc.z / fc);
  p.a = mk(1.0f, 1.0f, 1.0f);
  p.c = m;
  if ((flags & kDnAlbedo) && kind == 1u) {
    p.a = mk(albedo.x > 0.0f ? albedo.x : 1.0f, albedo.y > 0.0f ? albedo.y : 1.0f, albedo.z > 0.0f ? albedo.z : 1.0f);
    p.c = mk(m.x / p.a.x, m.y / p.a.y, m.z / p.a.z);
  }
  p.valid = cnt > 0 && dn_finite(p.c.x) && dn_finite(p.c.y) && dn_finite(p.c.z);
  if (!p.valid) {  // comes out (+0, +0, +0) whatever a' would be
    p.c = mk(0.0f, 0.0f, 0.0f);
    p.a = mk(1.0f, 1.0f, 1.0f);
  }
  return p;
}

// The weight of one non-centre tap q of a centre p that passed the valid and
// kind tests. h: the stencil weight; s2 = sig * sig; surf: kind[p] != 0;
// zden = (sigma_z * t_p) * (float)step. The caller keeps the tap if w > 0
// (which also drops the NaN of 0 / 0).
WPT_HD float dn_weight(float h, V3 cp, V3 cq, float s2, bool surf, V3 np, V3 nq, float tp, float tq, float zden) {
  const V3 dc = sub(cp, cq);
  const float l = (dc.x * dc.x + dc.y * dc.y) + dc.z * dc.z;
  float w = h * (1.0f / (1.0f + l / s2));
  if (surf) {
    float d = fmaxf((np.x * nq.x + np.y * nq.y) + np.z * nq.z, 0.0f);
    d = d * d;
    d = d * d;
    d = d * d;
    d = d * d;
    d = d * d;  // d^32
    w = w * d;
    const float dz = fabsf(tp - tq);
    const float r = dz / zden;
    w = w * (1.0f / (1.0f + r * r));
  }
  return w;
}

// render_target.rs:62-64: (clamp(v, 0, 1) * 255) as u8
WPT_HD uint8_t dn_quant(float v) { return (uint8_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }

struct DnTapSum {
  V3 a;
  float sw;
};
WPT_HD void dn_add(DnTapSum& s, float w, V3 cq) {
  s.a = mk(s.a.x + w * cq.x, s.a.y + w * cq.y, s.a.z + w * cq.z);
  s.sw = s.sw + w;
}

// The restatement on the host: the same functions, pixel by pixel. Its first
// half, the pack and the passes (iterations may be 0), is also the coarse stage
// of upsample_host (wpt_upsample.h): c the filtered value, ap = a', ok = valid.
struct DnHostFrame {
  std::vector<V3> c, ap;
  std::vector<uint8_t> ok;
};
inline void dn_host_passes(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, const float* t,
                           const float* normal3, const float* albedo3, const uint8_t* kind, uint32_t iterations,
                           float sigma_c, float sigma_z, uint32_t flags, DnHostFrame& F) {
  const size_t np = (size_t)W * H;
  std::vector<V3> c1(np);
  std::vector<V3>& c0 = F.c;
  std::vector<V3>& ap = F.ap;
  std::vector<uint8_t>& ok = F.ok;
  c0.resize(np);
  ap.resize(np);
  ok.resize(np);
  for (size_t i = 0; i < np; i++) {
    const DnPix p = dn_pack(mk(acc3[3 * i], acc3[3 * i + 1], acc3[3 * i + 2]), cnt[i],
                            mk(albedo3[3 * i], albedo3[3 * i + 1], albedo3[3 * i + 2]), kind[i], flags);
    c0[i] = p.c;
    ap[i] = p.a;
    ok[i] = p.valid ? 1 : 0;
  }
  float sig = sigma_c;
  for (uint32_t it = 0; it < iterations; it++) {
    const int step = 1 << it;
    const float s2 = sig * sig;
    for (int y = 0; y < (int)H; y++)
      for (int x = 0; x < (int)W; x++) {
        const size_t p = (size_t)y * W + x;
        if (!ok[p]) { c1[p] = mk(0.0f, 0.0f, 0.0f); continue; }
        const V3 cp = c0[p], n_p = mk(normal3[3 * p], normal3[3 * p + 1], normal3[3 * p + 2]);
        const bool surf = kind[p] != 0;
        const float tp = t[p], zden = (sigma_z * tp) * (float)step;
        DnTapSum s{mk(0.0f, 0.0f, 0.0f), 0.0f};
        for (int vy = 0; vy < 5; vy++)
          for (int vx = 0; vx < 5; vx++) {
            const int qx = x + (vx - 2) * step, qy = y + (vy - 2) * step;
            if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) continue;
            const size_t q = (size_t)qy * W + qx;
            float w = 36.0f;
            if (vy != 2 || vx != 2) {
              if (!ok[q] || kind[q] != kind[p]) continue;
              w = dn_weight(dn_gauss(vy, vx), cp, c0[q], s2, surf, n_p,
                            mk(normal3[3 * q], normal3[3 * q + 1], normal3[3 * q + 2]), tp, t[q], zden);
            }
            if (!(w > 0.0f)) continue;
            dn_add(s, w, c0[q]);
          }
        c1[p] = mk(s.a.x / s.sw, s.a.y / s.sw, s.a.z / s.sw);
      }
    c0.swap(c1);
    sig = sig * 0.5f;
  }
}

inline void denoise_host(uint32_t W, uint32_t H, const float* acc3, const uint32_t* cnt, const float* t,
                         const float* normal3, const float* albedo3, const uint8_t* kind, uint32_t iterations,
                         float sigma_c, float sigma_z, uint32_t flags, float* rgb3, uint8_t* valid, uint8_t* rgba) {
  DnHostFrame F;
  dn_host_passes(W, H, acc3, cnt, t, normal3, albedo3, kind, iterations, sigma_c, sigma_z, flags, F);
  const std::vector<V3>& c0 = F.c;
  const std::vector<V3>& ap = F.ap;
  const std::vector<uint8_t>& ok = F.ok;
  const size_t np = (size_t)W * H;
  for (size_t i = 0; i < np; i++) {
    const V3 o = mk(c0[i].x * ap[i].x, c0[i].y * ap[i].y, c0[i].z * ap[i].z);
    if (rgb3) { rgb3[3 * i] = o.x; rgb3[3 * i + 1] = o.y; rgb3[3 * i + 2] = o.z; }
    if (valid) valid[i] = ok[i];
    if (rgba) {
      rgba[4 * i] = dn_quant(o.x);
      rgba[4 * i + 1] = dn_quant(o.y);
      rgba[4 * i + 2] = dn_quant(o.z);
      rgba[4 * i + 3] = 255;
    }
  }
}

#if defined(WPT_DENOISE_KERNELS)

constexpr int kDnTile = 16;    // pixels per tile side: kDnTile^2 = kBlock lanes
constexpr int kDnPitch = 32;   // records per LDS row (see the header comment)
static_assert(kDnTile * kDnTile == (int)kBlock, "one lane per pixel of a tile");

// acc: the frame's float4 sums; t, normal, albedo, kind: k_first_hit's planes
__global__ void __launch_bounds__(kBlock) k_dn_pack(const float4* __restrict__ acc, const uint32_t* __restrict__ cnt,
                                                    const float* __restrict__ t, const float* __restrict__ normal,
                                                    const float* __restrict__ albedo, const uint8_t* __restrict__ kind,
                                                    uint32_t npix, uint32_t flags, float4* __restrict__ A,
                                                    float4* __restrict__ B, float* __restrict__ ap) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  const float4 a = acc[i];
  const uint32_t k = kind[i];
  const size_t j = 3 * (size_t)i;
  const DnPix p = dn_pack(mk(a.x, a.y, a.z), cnt[i], mk(albedo[j], albedo[j + 1], albedo[j + 2]), k, flags);
  A[i] = make_float4(p.c.x, p.c.y, p.c.z, t[i]);
  B[i] = make_float4(normal[j], normal[j + 1], normal[j + 2], __uint_as_float(k | (p.valid ? 0x100u : 0u)));
  st3(ap + j, p.a);
}

// One iteration: Aout = the filtered A (t carried along). s2 = sig * sig.
template <int STEP, bool LDS>
__global__ void __launch_bounds__(kBlock) k_dn_atrous(const float4* __restrict__ A, const float4* __restrict__ B,
                                                      uint32_t W, uint32_t H, float s2, float sigma_z,
                                                      float4* __restrict__ Aout) {
  constexpr int kHalo = 2 * STEP, kSide = kDnTile + 2 * kHalo;
  // a tile outside the viewport reads as invalid: never a tap
  __shared__ float4 sA[LDS ? kSide * kDnPitch : 1];
  __shared__ float4 sB[LDS ? kSide * kDnPitch : 1];
  const int tx0 = (int)blockIdx.x * kDnTile, ty0 = (int)blockIdx.y * kDnTile;
  if (LDS) {
    static_assert(!LDS || kSide <= kDnPitch, "a tile row fits the pitch");
    for (int k = threadIdx.x; k < kSide * kSide; k += kBlock) {
      const int sx = k % kSide, sy = k / kSide;
      const int px = tx0 - kHalo + sx, py = ty0 - kHalo + sy;
      float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
      if (px >= 0 && py >= 0 && px < (int)W && py < (int)H) {
        const size_t g = (size_t)py * W + (size_t)px;
        a = A[g];
        b = B[g];
      }
      sA[sy * kDnPitch + sx] = a;
      sB[sy * kDnPitch + sx] = b;
    }
    __syncthreads();
  }
  const int lx = (int)(threadIdx.x % kDnTile), ly = (int)(threadIdx.x / kDnTile);
  const int x = tx0 + lx, y = ty0 + ly;
  if (x >= (int)W || y >= (int)H) return;
  const size_t p = (size_t)y * W + (size_t)x;
  const int lc = (ly + kHalo) * kDnPitch + (lx + kHalo);
  const float4 ap = LDS ? sA[lc] : A[p], bp = LDS ? sB[lc] : B[p];
  const uint32_t mp = __float_as_uint(bp.w);  // kind | valid << 8
  if (!(mp & 0x100u)) {
    Aout[p] = make_float4(0.0f, 0.0f, 0.0f, ap.w);
    return;
  }
  const V3 cp = mk(ap.x, ap.y, ap.z), n_p = mk(bp.x, bp.y, bp.z);
  const bool surf = (mp & 0xFFu) != 0;
  const float tp = ap.w, zden = (sigma_z * tp) * (float)STEP;
  DnTapSum s{mk(0.0f, 0.0f, 0.0f), 0.0f};
#pragma unroll
  for (int vy = 0; vy < 5; vy++) {
#pragma unroll
    for (int vx = 0; vx < 5; vx++) {
      const int dx = (vx - 2) * STEP, dy = (vy - 2) * STEP;
      if (vy == 2 && vx == 2) {
        dn_add(s, 36.0f, cp);
        continue;
      }
      float4 aq, bq;
      if (LDS) {
        // the halo holds invalid records outside the viewport
        const int k = lc + dy * kDnPitch + dx;
        bq = sB[k];
        if (__float_as_uint(bq.w) != mp) continue;  // invalid, or another kind
        aq = sA[k];
      } else {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) continue;
        const size_t q = (size_t)qy * W + (size_t)qx;
        bq = B[q];
        if (__float_as_uint(bq.w) != mp) continue;
        aq = A[q];
      }
      const V3 cq = mk(aq.x, aq.y, aq.z);
      const float w = dn_weight(dn_gauss(vy, vx), cp, cq, s2, surf, n_p, mk(bq.x, bq.y, bq.z), tp, aq.w, zden);
      if (!(w > 0.0f)) continue;
      dn_add(s, w, cq);
    }
  }
  Aout[p] = make_float4(s.a.x / s.sw, s.a.y / s.sw, s.a.z / s.sw, tp);
}

// out = c * a'; a null output is not written
__global__ void __launch_bounds__(kBlock) k_dn_unpack(const float4* __restrict__ A, const float4* __restrict__ B,
                                                      const float* __restrict__ ap, uint32_t npix,
                                                      float* __restrict__ rgb, uint8_t* __restrict__ valid,
                                                      uint8_t* __restrict__ rgba) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  const float4 a = A[i];
  const size_t j = 3 * (size_t)i;
  const V3 o = mk(a.x * ap[j], a.y * ap[j + 1], a.z * ap[j + 2]);
  if (rgb) st3(rgb + j, o);
  if (valid) valid[i] = (__float_as_uint(B[i].w) & 0x100u) ? 1 : 0;
  if (rgba) reinterpret_cast<uchar4*>(rgba)[i] = make_uchar4(dn_quant(o.x), dn_quant(o.y), dn_quant(o.z), 255);
}

#endif  // WPT_DENOISE_KERNELS
