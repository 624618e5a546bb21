// wpt_first_hit_rays.h — first-hit feature planes along a caller's rays
// (wpt_first_hit_rays, include/wpt.h): wpt_first_hit.h's planes for rays that
// are not gen_path's, so that a frame of a camera the session does not know
// (fisheye, panorama, orthographic) gets the guide planes the filter reads
// (wpt_denoise_rays).
//
// Included by wpt_render.hip inside its anonymous namespace after
// wpt_first_hit.h (the plane bits kFh*, the traversal block's LDS layout) and
// wpt_rays.h (ray_valid), none of which it restates: the closest hit is
// begin_extend + step<…, REF_VISITS> on the exact BVH2, the normal hit_normal,
// the material S.mats, exactly as k_first_hit has them. Entry i of every plane
// is what k_first_hit gives a pixel whose primary ray is ray i.
//
// Lane mapping: one lane per ray, origin and direction per lane, read straight
// from the caller's 24-byte records (six dword loads per lane; no staging: the
// block's LDS is the traversal's whole budget, WPT_TREE_PAIRS). A wave takes 64
// consecutive rays; a block's waves take consecutive groups and, on a grid
// clamped by the spill area, further ones a grid stride on. Lanes past n and
// lanes whose ray ray_valid rejects never start a ray but stay in the wave's
// loop, so the machine's wave-wide tests see the whole wave; a wave with no
// valid ray leaves at once. An invalid ray's entries are the miss entries with
// visits 0. (Measured and dropped: a wave per 8 x 8 tile of a W x H grid of
// rays, k_first_hit's mapping. C3 at 1080p, device ms: 0.331 for the list,
// 0.345 tiled, 0.346 k_first_hit itself, the ranges overlapping,
// profiles/rayframe/README.md.)
//
// Resources: the block is k_first_hit's (launch bounds, 19,920 B of LDS, 8 and
// 6 waves per SIMD); without GenParams in the argument block the triangle
// variant has no scratch (k_first_hit<true>: 36 B per lane).
#pragma once

struct FirstHitRaysParams {
  const float* rays;  // 6 f32 per ray {ox,oy,oz,dx,dy,dz}
  uint32_t n;
  uint32_t ngroups;   // waves' worth of rays: ceil(n / 64)
  uint32_t mask;      // kFh* (never kFhDir): the planes wanted
  float* t;
  int32_t* id;
  uint32_t* visits;
  float* normal;      // 3 per ray
  float* albedo;      // 3 per ray
  uint8_t* kind;
};

// The filter's counts of a frame of query rays (wpt_denoise_rays): spp samples
// where the ray was traced, none where it was not. Stated from the status, not
// read from the query's count buffer.
__global__ void __launch_bounds__(kBlock) k_rayframe_cnt(uint32_t n, const uint8_t* __restrict__ status, uint32_t spp,
                                                         uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  cnt[i] = spp * status[i];
}

template <bool TRI_ONLY>
__global__ void WPT_TRACE_BOUNDS k_first_hit_rays(DevScene S, FirstHitRaysParams P, uint2* __restrict__ spill) {
  __shared__ uint32_t s_code[kLdsSlots * kTBlock];
  __shared__ float s_h[kLdsSlots * kTBlock];
  __shared__ float s_lrec[16 * kLdsLights];
  __shared__ int32_t s_lid[kLdsLights];
  __shared__ f4v s_tree[4 * kTreePairs + 1];
  const Hot H = load_hot(S, (lds_f32h*)s_lrec, (lds_i32*)s_lid, (lds_f4v*)s_tree, (const float4*)s_tree);
  const uint32_t G = gridDim.x * kTBlock;
  const Stack stk{(lds_u32*)(s_code + threadIdx.x), (lds_f32*)(s_h + threadIdx.x),
                  spill + blockIdx.x * kTBlock + threadIdx.x, G, S.stack_cap, S.overflow};
  constexpr uint32_t kWaves = kTBlock / 64;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const float inf = __int_as_float(0x7f800000);
  // wave-uniform: every lane of a wave makes the same trips
  for (uint32_t grp = blockIdx.x * kWaves + wave; grp < P.ngroups; grp += gridDim.x * kWaves) {
    const uint32_t i = grp * 64u + lane;  // < 2^32: grp * 64 <= n - 1
    const bool in = i < P.n;
    float c[6];
    for (int k = 0; k < 6; k++) c[k] = in ? P.rays[6 * (size_t)i + k] : 0.0f;
    const bool ok = in && ray_valid(c);
    uint32_t visits = 0, tests = 0, nbytes = 0;
    bool dummy = false;
    Lane L;
    L.best = inf;
    L.best_id = -1;
    bool live = false;
    if (ok) live = begin_extend<TRI_ONLY, true, false>(S, H, L, mk(c[0], c[1], c[2]), mk(c[3], c[4], c[5]), visits, tests, nbytes);
    while (__any(live)) {
      if (live) live = step<false, TRI_ONLY, true, false, true>(S, H, L, stk, -1, 0.0f, dummy, visits, tests, nbytes);
    }
    if (!in) continue;
    const int32_t id = L.best_id;
    const bool hit = id >= 0;  // an invalid ray: never
    const float t = hit ? L.best : inf;
    if (P.mask & kFhT) P.t[i] = t;
    if (P.mask & kFhId) P.id[i] = id;
    if (P.mask & kFhVisits) P.visits[i] = visits;
    if (P.mask & kFhNormal) {
      V3 n = mk(0.0f, 0.0f, 0.0f);
      if (hit) n = hit_normal<TRI_ONLY>(S, id, L.o, L.d, t);  // (begin_extend's copies: not held twice across the walk)
      st3(P.normal + 3 * (size_t)i, n);
    }
    if (P.mask & (kFhAlbedo | kFhKind)) {
      float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (hit) m = S.mats[id];
      if (P.mask & kFhAlbedo) st3(P.albedo + 3 * (size_t)i, ld3(m));
      if (P.mask & kFhKind) P.kind[i] = hit ? (m.w != 0.0f ? 2 : 1) : 0;
    }
  }
}
